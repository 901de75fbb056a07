// Policy entropy and KL against a reference model for given rows.
//
// For row n and attribute a, with x the model's logits and y a reference model's (PAIR): p = softmax(x), p' =
// softmax(y) (temperature 1, no mask, no nucleus) and q, q' the distributions the device sampler (csrc/sample.hip)
// draws from on x and on y: tempered logits, the constraint mask row, the row grammar, the nucleus kept set,
// renormalised.  Out, f32 nats: {H(p), H(q)} or {H(p), H(q), KL(p || p'), KL(q || q')}.
//
// The sampler's layout: one workgroup per row, one wave per attribute, lane l owns classes 4l .. 4l + 3, the per-wave
// LDS row for the nucleus ranking; no workgroup barriers, no atomics.  The support rule (allowed classes, kept set) is
// restated from draw_attr with the same operations in the same order, so the kept set is the sampler's bit for bit
// (tests/test_policy_stats_gpu.py holds it to the scorer class by class).
//
// Arithmetic: every sum is term by term over the kept set K, H = sum q_j * t_j with t_j = log S - (v_j - m) >= 0 and
// KL = sum q_j * (l_j - l'_j), both log-probabilities formed from the logits, l_j = (v_j - m) - log S: no logarithm of
// an exponentiated value, so a reference probability that underflows in f32 still has a finite log.  Classes outside K
// are never multiplied.  KL(q || q') = +inf when K is not inside K'; with no allowed class at all (an ill-formed row
// under a grammar) the sampler columns are NaN and the model columns stay finite.
#include "cwlt_common.h"

#define CWLT_STATS_MAX_ATTR 8

namespace cwlt {

struct StatsArgs {
    int n[CWLT_STATS_MAX_ATTR];
    int off[CWLT_STATS_MAX_ATTR];
    float inv_t[CWLT_STATS_MAX_ATTR];                // 1 / temperature per attribute
    float top_p[CWLT_STATS_MAX_ATTR];                // nucleus mass per attribute; >= 1: plain categorical
};

// The constraint table of cwlt_score_categorical: row n's song is key[n] (n without keys), its mask row sched[2k] +
// min(bar[n] - 1, sched[2k + 1] - 1).
struct StatsMask {
    const int64_t* key;
    const int64_t* bar;
    const int64_t* sched;
    const uint32_t* masks;
    long n_sched, rows;
    int words;
};

// The row grammar of cwlt_score_categorical_grammar: beat[n] the position before the row, order / gram its tables.
struct StatsGrammar {
    const int64_t* beat;
    const int* order;
    const uint32_t* gram;
    int words;
    int bar_attr;
};

constexpr int STATS_KIND_NONE = -1;                  // an ill-formed row: nothing is allowed
constexpr int STATS_KIND_POSITION = 3;               // the bar-beat attribute itself: the position rule, no gram row

__device__ __forceinline__ int stats_kind(int o) { return o == -2 ? 0 : o == -1 ? 1 : o >= 0 ? 2 : STATS_KIND_NONE; }

// The classes of attribute a the sampler may draw in row n (draw_attr's mask and grammar rules) -> ok.
template <bool MASKED, bool GRAMMAR>
__device__ __forceinline__ void stats_allowed(const StatsArgs& A, const StatsMask& M, const StatsGrammar& G, int n,
                                              int lane, int a, int kind, bool ok[4]) {
    const int nc = A.n[a];
#pragma unroll
    for (int j = 0; j < 4; ++j) ok[j] = true;
    if constexpr (MASKED) {
        const long k = M.key ? M.key[n] : (long)n;
        if (k >= 0 && k < M.n_sched) {
            const long first = M.sched[2 * k], len = M.sched[2 * k + 1];
            long b = M.bar[n] - 1;
            b = b < 0 ? 0 : b < len - 1 ? b : len - 1;
            const long r = first + b;
            if (len > 0 && r >= 0 && r < M.rows) {
                const uint32_t* w = M.masks + r * M.words;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int bit = A.off[a] + lane * 4 + j;         // < sum n_class <= 32 * words: inside the row
                    ok[j] = lane * 4 + j < nc ? ((w[bit >> 5] >> (bit & 31)) & 1u) != 0 : false;
                }
            }
        }
    }
    if constexpr (GRAMMAR) {
        if (kind == STATS_KIND_POSITION) {
            const long bt = G.beat[n];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = lane * 4 + j;
                if (c < nc) {
                    const int o = G.order[c];        // order holds >= nc entries (checked by the entry point)
                    ok[j] = ok[j] && (o == -1 || (o >= 0 && o > bt) || (o == -2 && bt >= 0));
                }
            }
        } else {
            const uint32_t* w = G.gram + (kind < 0 ? 0 : kind) * G.words;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int bit = A.off[a] + lane * 4 + j;             // < sum n_class <= 32 * words: inside the row
                if (lane * 4 + j < nc) ok[j] = ok[j] && kind >= 0 && ((w[bit >> 5] >> (bit & 31)) & 1u) != 0;
            }
        }
    }
}

// One distribution of the wave's attribute: v the logits it is a softmax of (-inf outside the allowed classes), m
// their max, e = exp(v - m) on the kept set K and 0 elsewhere, keep = K, S = sum of e over K.
struct StatsDist {
    float v[4], e[4];
    bool keep[4];
    float m, S;
};

// The sampler's distribution on logits x: draw_attr's v, m, e, and its nucleus ranking through the wave's LDS row ew.
__device__ __forceinline__ void stats_sampler_dist(const float* __restrict__ x, float inv_t, float top_p, int nc,
                                                   int lane, const bool ok[4], float* ew, StatsDist& d) {
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane * 4 + j;
        d.v[j] = c < nc && ok[j] ? x[c] * inv_t : -INFINITY;
        m = fmaxf(m, d.v[j]);
    }
    m = wave_max(m);
    float e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = lane * 4 + j < nc && ok[j] ? expf(d.v[j] - m) : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) d.keep[j] = lane * 4 + j < nc && ok[j];
    if (top_p < 1.0f) {
        // the kept set of the nucleus: the mass ranked ahead of class i (larger e, ties: the larger index first) is
        // <= top_p * tot * (1 + 1e-5)
#pragma unroll
        for (int j = 0; j < 4; ++j) ew[lane * 4 + j] = e[j];
        float tot = (e[0] + e[1]) + (e[2] + e[3]);
        tot = wave_sum(tot);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        float ahead[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < nc; ++c) {
            const float ec = ew[c];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = lane * 4 + j;
                ahead[j] += (ec > e[j] || (ec == e[j] && c > i)) ? ec : 0.f;
            }
        }
        const float limit = top_p * (tot * (1.0f + 1e-5f));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            e[j] = ahead[j] <= limit ? e[j] : 0.f;
            d.keep[j] = d.keep[j] && ahead[j] <= limit;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) d.e[j] = d.keep[j] ? e[j] : 0.f;
    d.m = m;
    d.S = wave_sum((d.e[0] + d.e[1]) + (d.e[2] + d.e[3]));
}

// The model's distribution on logits x: the raw logits of every class of the attribute.
__device__ __forceinline__ void stats_model_dist(const float* __restrict__ x, int nc, int lane, StatsDist& d) {
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
// left unwritten.  out: rows x n_attr x (PAIR ? 4 : 2) f32.
template <bool MASKED, bool GRAMMAR, bool PAIR>
__global__ __launch_bounds__(64 * CWLT_STATS_MAX_ATTR) void policy_stats_kernel(
    const float* __restrict__ logits, long ld, const float* __restrict__ ref, long ref_ld, StatsArgs A, int n_attr,
    const int64_t* __restrict__ bar_class, StatsMask M, StatsGrammar G, float* __restrict__ out) {
    __shared__ float e_s[CWLT_STATS_MAX_ATTR][256];
    const int lane = threadIdx.x & 63, a = threadIdx.x >> 6, n = blockIdx.x;
    if (a >= n_attr) return;                         // wave-uniform; no workgroup barriers in this kernel
    const long bc = bar_class ? bar_class[n] : 0;
    if (bc < 0) return;                              // padding row: wave-uniform, nothing written
    int kind = STATS_KIND_POSITION;
    if constexpr (GRAMMAR)
        if (a != G.bar_attr) kind = bc < A.n[G.bar_attr] ? stats_kind(G.order[bc]) : STATS_KIND_NONE;
    const int nc = A.n[a];
    bool ok[4];
    stats_allowed<MASKED, GRAMMAR>(A, M, G, n, lane, a, kind, ok);
    bool any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) any = any || (lane * 4 + j < nc && ok[j]);
    const bool empty = __ballot(any) == 0;           // no allowed class: the sampler columns are NaN

    const float* x = logits + (long)n * ld + A.off[a];
    StatsDist p, q;
    stats_model_dist(x, nc, lane, p);
    stats_sampler_dist(x, A.inv_t[a], A.top_p[a], nc, lane, ok, e_s[a], q);
    const float hp = stats_entropy(p);
    const float hq = empty ? NAN : stats_entropy(q);
    float* o = out + ((long)n * n_attr + a) * (PAIR ? 4 : 2);
    if constexpr (!PAIR) {
        if (lane == 0) *reinterpret_cast<float2*>(o) = make_float2(hp, hq);
    } else {
        const float* y = ref + (long)n * ref_ld + A.off[a];
        StatsDist pr, qr;
        stats_model_dist(y, nc, lane, pr);
        __builtin_amdgcn_wave_barrier();             // the LDS row is reused: reads above stay before the writes below
        stats_sampler_dist(y, A.inv_t[a], A.top_p[a], nc, lane, ok, e_s[a], qr);
        const float kp = stats_kl(p, pr);
        const float kq = empty ? NAN : stats_kl(q, qr);
        if (lane == 0) *reinterpret_cast<float4*>(o) = make_float4(hp, hq, kp, kq);
    }
}

}  // namespace cwlt

template <bool MASKED, bool GRAMMAR, bool PAIR>
static void launch_policy_stats(int64_t rows, int n_attr, void* stream, const float* logits, int64_t ld,
                                const float* ref, int64_t ref_ld, const cwlt::StatsArgs& A, const int64_t* bar_class,
                                const cwlt::StatsMask& M, const cwlt::StatsGrammar& G, float* out) {
    hipLaunchKernelGGL((cwlt::policy_stats_kernel<MASKED, GRAMMAR, PAIR>), dim3((unsigned)rows), dim3(64 * n_attr), 0,
                       (hipStream_t)stream, logits, (long)ld, ref, (long)ref_ld, A, n_attr, bar_class, M, G, out);
}

extern "C" int cwlt_policy_stats(const float* logits, const int* n_class, const float* temperature, const float* top_p,
                                 int n_attr, int64_t rows, int64_t ld, const float* ref_logits, int64_t ref_ld,
                                 const int64_t* bar_class, const int64_t* key, const int64_t* bar, const int64_t* sched,
                                 int64_t n_sched, const uint32_t* masks, int64_t mask_rows, int mask_words,
                                 const int64_t* beat, const int* order, int n_order, const uint32_t* gram,
                                 int gram_words, int bar_attr, float* out, void* stream) {
    using namespace cwlt;
    if (!logits || !n_class || !out || n_attr <= 0 || n_attr > CWLT_STATS_MAX_ATTR || rows <= 0 || rows > (1L << 20))
        return CWLT_ERR_ARG;
    StatsArgs A;
    int off = 0;
    for (int a = 0; a < n_attr; ++a) {
        if (n_class[a] <= 0 || n_class[a] > 256) return CWLT_ERR_ARG;
        if (temperature && !(temperature[a] > 0.f)) return CWLT_ERR_ARG;
        A.n[a] = n_class[a];
        A.off[a] = off;
        A.inv_t[a] = temperature ? 1.0f / temperature[a] : 1.0f;
        A.top_p[a] = top_p ? top_p[a] : 1.0f;
        if (!(A.top_p[a] > 0.f)) return CWLT_ERR_ARG;
        off += n_class[a];
    }
    if (ld < off || (ref_logits && ref_ld < off)) return CWLT_ERR_ARG;
    const bool masked = bar || sched || masks;       // all of the table, or none of it
    if (masked && (!bar || !sched || !masks || n_sched < 1 || mask_rows < 1 || mask_words < 1)) return CWLT_ERR_ARG;
    if (masked && (int64_t)mask_words * 32 < off) return CWLT_ERR_ARG;
    const bool grammar = beat || order || gram;
    if (grammar) {
        if (!beat || !order || !gram || gram_words < 1 || bar_attr < 0 || bar_attr >= n_attr) return CWLT_ERR_ARG;
        if (n_order < n_class[bar_attr] || (int64_t)gram_words * 32 < off) return CWLT_ERR_ARG;
        if (!bar_class) return CWLT_ERR_ARG;         // the row's own bar-beat class fixes its kind
    }
    const StatsMask M = masked ? StatsMask{key, bar, sched, masks, (long)n_sched, (long)mask_rows, mask_words}
                               : StatsMask{};
    const StatsGrammar G = grammar ? StatsGrammar{beat, order, gram, gram_words, bar_attr} : StatsGrammar{};
#define CWLT_STATS_LAUNCH(MK, GR, PR)                                                                                 \
    launch_policy_stats<MK, GR, PR>(rows, n_attr, stream, logits, ld, ref_logits, ref_ld, A, bar_class, M, G, out)
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
