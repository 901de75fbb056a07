// Policy entropy and KL against a reference model for given rows.
//
// For row n and attribute a, with x the model's logits and y a reference model's (PAIR): p = softmax(x), p' =
// softmax(y) (temperature 1, no mask, no nucleus) and q, q' the distributions the device sampler (csrc/sample.hip)
// draws from on x and on y: tempered logits, the constraint mask row, the row grammar, the nucleus kept set,
// renormalised.  Out, f32 nats: {H(p), H(q)} or {H(p), H(q), KL(p || p'), KL(q || q')}.
//
// The sampler's layout: one workgroup per row, one wave per attribute, lane l owns classes 4l .. 4l + 3, the per-wave
// LDS row for the nucleus ranking; no workgroup barriers, no atomics.  The support rule (allowed classes, kept set) is
// the sampler's own code, allowed_classes and sampler_support of cwlt_sampler_support.h, so the kept set is the
// sampler's bit for bit (tests/test_policy_stats_gpu.py holds it to the scorer class by class).
//
// Arithmetic: every sum is term by term over the kept set K, H = sum q_j * t_j with t_j = log S - (v_j - m) >= 0 and
// KL = sum q_j * (l_j - l'_j), both log-probabilities formed from the logits, l_j = (v_j - m) - log S: no logarithm of
// an exponentiated value, so a reference probability that underflows in f32 still has a finite log.  Classes outside K
// are never multiplied.  KL(q || q') = +inf when K is not inside K'; with no allowed class at all (an ill-formed row
// under a grammar) the sampler columns are NaN and the model columns stay finite.
#include "cwlt_sampler_support.h"

namespace cwlt {

// One distribution of the wave's attribute: v the logits it is a softmax of (-inf outside the allowed classes), m
// their max, e = exp(v - m) on the kept set K and 0 elsewhere, keep = K, S = sum of e over K.
struct StatsDist {
    float v[4], e[4];
    bool keep[4];
    float m, S;
};

// The sampler's distribution on logits x over the allowed classes ok, through the wave's LDS row ew.
__device__ __forceinline__ StatsDist stats_sampler_dist(const float* __restrict__ x, const SampleArgs& A, int a, int nc,
                                                        int lane, const bool (&ok)[4], float* ew) {
    const SamplerSupport s = sampler_support<true>(x, A, a, nc, lane, ok[0], ok[1], ok[2], ok[3], ew);
    StatsDist d;
#pragma unroll
    for (int j = 0; j < 4; ++j) d.v[j] = s.v[j], d.e[j] = s.e[j], d.keep[j] = s.keep[j];
    d.m = s.m;
    d.S = wave_sum((d.e[0] + d.e[1]) + (d.e[2] + d.e[3]));
    return d;
}

// The model's distribution on logits x: the raw logits of every class of the attribute.
__device__ __forceinline__ StatsDist stats_model_dist(const float* __restrict__ x, int nc, int lane) {
    StatsDist d;
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        d.keep[j] = lane * 4 + j < nc;
        d.v[j] = d.keep[j] ? x[lane * 4 + j] : -INFINITY;
        m = fmaxf(m, d.v[j]);
    }
    m = wave_max(m);
#pragma unroll
    for (int j = 0; j < 4; ++j) d.e[j] = d.keep[j] ? expf(d.v[j] - m) : 0.f;
    d.m = m;
    d.S = wave_sum((d.e[0] + d.e[1]) + (d.e[2] + d.e[3]));
    return d;
}

// H = sum over K of q_j * t_j, q_j = e_j / S, t_j = log S - (v_j - m).
__device__ __forceinline__ float stats_entropy(const StatsDist& d) {
    const float ls = logf(d.S);
    float h = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (d.keep[j]) h += (d.e[j] / d.S) * (ls - (d.v[j] - d.m));
    return wave_sum(h);
}

// KL(d || r) = sum over K of q_j * (l_j - l'_j); +inf when a class of K is outside K'.
__device__ __forceinline__ float stats_kl(const StatsDist& d, const StatsDist& r) {
    const float ls = logf(d.S), lr = logf(r.S);
    float kl = 0.f;
    bool out = false;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (d.keep[j]) {
            out = out || !r.keep[j];
            if (r.keep[j]) kl += (d.e[j] / d.S) * (((d.v[j] - d.m) - ls) - ((r.v[j] - r.m) - lr));
        }
    kl = wave_sum(kl);
    return __ballot(out) != 0 ? INFINITY : kl;
}

// bar_class[n] (nullable): the row's own bar-beat class, the kind of the row under a grammar; negative: a padding row,
// left unwritten.  key (nullable): the song of each row for the constraint table M, as the scorers' (NULL: row n is
// song n).  out: rows x n_attr x (PAIR ? 4 : 2) f32.
template <bool MASKED, bool GRAMMAR, bool PAIR>
__global__ __launch_bounds__(64 * CWLT_MAX_ATTR) void policy_stats_kernel(
    const float* __restrict__ logits, long ld, const float* __restrict__ ref, long ref_ld, SampleArgs A, int n_attr,
    const int64_t* __restrict__ bar_class, const int64_t* __restrict__ key, MaskArgs M, GrammarArgs G,
    float* __restrict__ out) {
    __shared__ float e_s[CWLT_MAX_ATTR][256];
    const int lane = threadIdx.x & 63, a = threadIdx.x >> 6, n = blockIdx.x;
    if (a >= n_attr) return;                         // wave-uniform; no workgroup barriers in this kernel
    const long bc = bar_class ? bar_class[n] : 0;
    if (bc < 0) return;                              // padding row: wave-uniform, nothing written
    int kind = KIND_POSITION;
    if constexpr (GRAMMAR)
        if (a != G.bar_attr) kind = bc < A.n[G.bar_attr] ? grammar_kind(G.order[bc]) : KIND_NONE;
    const int nc = A.n[a];
    // The model's distributions first, then the allowed classes and the sampler's: the statement order is part of the
    // kernels' schedule and was chosen by timing all eight forms (HISTORY §14).
    const float* x = logits + (long)n * ld + A.off[a];
    const StatsDist p = stats_model_dist(x, nc, lane);
    const float* y = PAIR ? ref + (long)n * ref_ld + A.off[a] : x;
    StatsDist pr;                                    // the reference model's: PAIR only
    if constexpr (PAIR) pr = stats_model_dist(y, nc, lane);
    const AllowedClasses al = allowed_classes<MASKED, GRAMMAR>(A, M, G, key, n, lane, a, kind);
    const bool(&ok)[4] = al.ok;
    const StatsDist q = stats_sampler_dist(x, A, a, nc, lane, ok, e_s[a]);
    bool any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) any = any || (lane * 4 + j < nc && ok[j]);
    const bool empty = __ballot(any) == 0;           // no allowed class: the sampler columns are NaN

    const float hp = stats_entropy(p);
    const float hq = empty ? NAN : stats_entropy(q);
    float* o = out + ((long)n * n_attr + a) * (PAIR ? 4 : 2);
    if constexpr (!PAIR) {
        if (lane == 0) *reinterpret_cast<float2*>(o) = make_float2(hp, hq);
    } else {
        __builtin_amdgcn_wave_barrier();             // the LDS row is reused: reads above stay before the writes below
        const StatsDist qr = stats_sampler_dist(y, A, a, nc, lane, ok, e_s[a]);
        const float kp = stats_kl(p, pr);
        const float kq = empty ? NAN : stats_kl(q, qr);
        if (lane == 0) *reinterpret_cast<float4*>(o) = make_float4(hp, hq, kp, kq);
    }
}

}  // namespace cwlt

template <bool MASKED, bool GRAMMAR, bool PAIR>
static void launch_policy_stats(int64_t rows, int n_attr, void* stream, const float* logits, int64_t ld,
                                const float* ref, int64_t ref_ld, const cwlt::SampleArgs& A, const int64_t* bar_class,
                                const int64_t* key, const cwlt::MaskArgs& M, const cwlt::GrammarArgs& G, float* out) {
    hipLaunchKernelGGL((cwlt::policy_stats_kernel<MASKED, GRAMMAR, PAIR>), dim3((unsigned)rows), dim3(64 * n_attr), 0,
                       (hipStream_t)stream, logits, (long)ld, ref, (long)ref_ld, A, n_attr, bar_class, key, M, G, out);
}

extern "C" int cwlt_policy_stats(const float* logits, const int* n_class, const float* temperature, const float* top_p,
                                 int n_attr, int64_t rows, int64_t ld, const float* ref_logits, int64_t ref_ld,
                                 const int64_t* bar_class, const int64_t* key, const int64_t* bar, const int64_t* sched,
                                 int64_t n_sched, const uint32_t* masks, int64_t mask_rows, int mask_words,
                                 const int64_t* beat, const int* order, int n_order, const uint32_t* gram,
                                 int gram_words, int bar_attr, float* out, void* stream) {
    using namespace cwlt;
    if (!logits || !out || rows <= 0 || rows > (1L << 20)) return CWLT_ERR_ARG;
    SampleArgs A;
    int width = 0;
    if (sample_args(n_class, temperature, top_p, n_attr, ld, &A, &width)) return CWLT_ERR_ARG;
    if (ref_logits && ref_ld < width) return CWLT_ERR_ARG;
    MaskArgs M{};
    bool masked = false;                             // all of the table, or none of it
    if (mask_args(bar, sched, n_sched, masks, mask_rows, mask_words, &M, &masked)) return CWLT_ERR_ARG;
    if (masked && table_words(mask_words, width)) return CWLT_ERR_ARG;
    const bool grammar = beat || order || gram;
    const GrammarArgs G = grammar ? GrammarArgs{beat, order, gram, gram_words, bar_attr} : GrammarArgs{};
    if (grammar && (grammar_args(G, n_order, n_class, n_attr, width) || !bar_class))
        return CWLT_ERR_ARG;                         // bar_class: the row's own bar-beat class fixes its kind
    if (!masked) key = nullptr;
#define CWLT_STATS_LAUNCH(MK, GR, PR)                                                                                 \
    launch_policy_stats<MK, GR, PR>(rows, n_attr, stream, logits, ld, ref_logits, ref_ld, A, bar_class, key, M, G, out)
#define CWLT_STATS_FORM(PR)                                                                                           \
    do {                                                                                                              \
        if (grammar) {                                                                                                \
            if (masked) CWLT_STATS_LAUNCH(true, true, PR);                                                            \
            else CWLT_STATS_LAUNCH(false, true, PR);                                                                  \
        } else {                                                                                                      \
            if (masked) CWLT_STATS_LAUNCH(true, false, PR);                                                           \
            else CWLT_STATS_LAUNCH(false, false, PR);                                                                 \
        }                                                                                                             \
    } while (0)
    if (ref_logits)
        CWLT_STATS_FORM(true);
    else
        CWLT_STATS_FORM(false);
#undef CWLT_STATS_FORM
#undef CWLT_STATS_LAUNCH
    return (int)hipGetLastError();
}
