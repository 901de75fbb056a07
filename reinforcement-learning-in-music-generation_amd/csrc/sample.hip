// Device-side categorical sampling of the next CW token -- the sampling half of the reference's PPO-side
// generation loop (/root/reference/ppo_policy/inference.py:115-141: softmax of each attribute's logits,
// torch.distributions.Categorical(...).sample(), actions concatenated and fed back as the next input).
//
// ... and of the DQN-side loop's samplers (dqn_policy/model.py:19-55,281-286: temperature, nucleus) when the caller
// asks for device-side sampling.
//
// One workgroup per song, one wave per attribute: softmax (max / sum by DPP reductions), inclusive prefix sum of
// the probabilities (lane-blocked layout: lane l owns classes 4l .. 4l+3, so class order == lane order), one
// uniform draw from the counter-based generator of cwlt_common.h keyed by (seed, draw counter, song, attribute),
// first class whose cumulative mass exceeds u * total.  The chosen ids go straight into the decode step's token
// buffer (and, optionally, row `counter` of the song), so a generation loop needs no host round trip per token.
// The draw counter is a device int64 read by the kernel: a captured hipGraph draws fresh numbers on every replay.
// Same distribution as the reference's sampler, not the same stream (torch's Philox stream is device- and
// version-specific anyway).
//
// Log-probabilities: the LOGP instantiations also write, per drawn class c, the pair (log_softmax of the
// raw logits at c, log q(c)) with q the distribution the draw was made from (temperature, mask, nucleus kept set,
// renormalised); the FORCED instantiations take c from a target array instead of drawing it and compute the same pair,
// through the same body, so scoring the logits a draw came from at the class it drew gives the sampler's bits.
//
// Row grammar: the GRAMMAR instantiations tie the attributes of a row together.  The bar-beat class is
// drawn under the position rule (GrammarArgs: beat, order) and decides the row's kind (NOTE / BAR / BEAT); every other
// attribute is drawn under the kind's row of `gram`.  Each wave of another attribute first runs the draw body on the
// bar-beat logits with bar-beat's own key and masks -- the very instructions the bar-beat wave runs, so all waves hold
// the same class -- and then runs it again for its own attribute: no workgroup barrier, no hand-off through memory.
#include "cwlt_sampler_support.h"

#include <climits>

namespace cwlt {

// Log-prob output of the LOGP / FORCED instantiations (unused otherwise; it is the last kernel argument, so the
// other arguments keep their offsets).  The pair of row n, attribute a goes to logp[((o * rows + n) * n_attr + a) * 2]
// with o = *out_counter % out_rows (o = 0 without a counter).  FORCED: the class is targets[n * n_attr + a]; a negative
// target (padding) leaves the pair unwritten.
struct LogpArgs {
    float* logp;
    const int64_t* out_counter;
    long out_rows;
    const int64_t* targets;
};

// The draw of attribute a of row n by one wave (lane-blocked: lane l owns classes 4l .. 4l + 3), `ew` the wave's LDS
// row -> the class.  write = false (GRAMMAR: another attribute's wave finding the row's bar-beat class) draws and
// writes nothing.  kind (GRAMMAR): KIND_POSITION for the bar-beat attribute, else the gram row, KIND_NONE = no class.
template <bool MASKED, bool LOGP, bool FORCED, bool GRAMMAR>
__device__ __forceinline__ int draw_attr(const float* __restrict__ logits, long ld, const SampleArgs& A, int n_attr,
                                         uint64_t seed, const int64_t* __restrict__ counter,
                                         int64_t* __restrict__ tokens, int64_t* __restrict__ song, long song_rows,
                                         int slot_keyed, const int64_t* __restrict__ row_key,
                                         const int64_t* __restrict__ row_step, const MaskArgs& M, const LogpArgs& L,
                                         const GrammarArgs& G, float* ew, int n, int lane, int a, long forced,
                                         bool write, int kind) {
    const int nc = A.n[a];
    const float* x = logits + (long)n * ld + A.off[a];
    // keyed by row: row n draws what the slot-keyed launch draws for row row_key[n] at counter row_step[n]
    const long step = FORCED ? 0 : row_step ? row_step[n] : counter ? *counter : 0;
    const AllowedClasses al = allowed_classes<MASKED, GRAMMAR>(A, M, G, row_key, n, lane, a, kind);
    const bool(&ok)[4] = al.ok;
    bool row_masked = al.row_masked;
    if constexpr (GRAMMAR && LOGP) row_masked = row_masked || __ballot(al.cut) != 0;   // permissive tables: the plain pair
    const SamplerSupport sup = sampler_support<LOGP>(x, A, a, nc, lane, ok[0], ok[1], ok[2], ok[3], ew);
    const float v[4] = {sup.v[0], sup.v[1], sup.v[2], sup.v[3]};
    float e[4] = {sup.e[0], sup.e[1], sup.e[2], sup.e[3]};
    const bool(&keep)[4] = sup.keep;                 // the support of q
    const float m = sup.m, tot_all = sup.tot_all;    // tot_all: the sum of e before the nucleus cut (nucleus rows only)
    float run = 0.f, cum[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        run += e[j];
        cum[j] = run;                                // inclusive within the lane
    }
    // exclusive prefix over lanes (Hillis-Steele on the lane totals)
    float inc = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    const float before = inc - run;
    const float total = lane_value(inc, 63);
    int pick = INT_MAX;
    if constexpr (FORCED) {
        pick = forced < nc ? (int)forced : INT_MAX;  // a class outside the attribute: both log-probs -inf
    } else {
        // slot-keyed: song n's draws do not depend on how many songs share the launch (the same keys at n = 0)
        const uint64_t slot = row_key ? (uint64_t)row_key[n] : (uint64_t)n;
        const uint64_t key = slot_keyed ? (slot << 40) + (uint64_t)step : (uint64_t)step * gridDim.x + n;
        const uint32_t r = rng_pair(seed, key * CWLT_MAX_ATTR + a);
        const float u = (float)(r >> 8) * (1.0f / 16777216.0f);      // [0, 1)
        const float target = u * total;
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            const int c = lane * 4 + j;
            if (c < nc && e[j] > 0.f && before + cum[j] > target) pick = c;
        }
        // the first lane (lowest classes) whose cumulative mass passes the target wins
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) pick = min(pick, __shfl_xor(pick, d, 64));
        if (pick == INT_MAX) {                       // u * total rounded past the last kept class: take that class
            int last = -1;
#pragma unroll
            for (int j = 0; j < 4; ++j) last = e[j] > 0.f ? lane * 4 + j : last;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) last = max(last, __shfl_xor(last, d, 64));
            pick = last < 0 ? 0 : last;
        }
        if (lane == 0 && write) {
            tokens[(long)n * n_attr + a] = pick;
            if (song && step < song_rows) song[((long)step * gridDim.x + n) * n_attr + a] = pick;
        }
    }
    if (LOGP && write) {
        // model log-prob: the raw logits' max and sum, or the sampler's own when they are the same numbers
        float mx = m, sx;
        if (A.inv_t[a] == 1.0f && !row_masked) {
            sx = A.top_p[a] < 1.0f ? tot_all : total;
        } else {
            float w[4];
            mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                w[j] = lane * 4 + j < nc ? x[lane * 4 + j] : -INFINITY;
                mx = fmaxf(mx, w[j]);
            }
            mx = wave_max(mx);
            float s4 = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) s4 += lane * 4 + j < nc ? expf(w[j] - mx) : 0.f;
            sx = wave_sum(s4);
        }
        // the picked class's lane holds its tempered logit and kept bit; one bpermute brings them to every lane
        float lq = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (lane * 4 + j == pick && keep[j]) lq = (v[j] - m) - logf(total);
        const int owner = pick < nc ? pick >> 2 : 0;
        lq = __shfl(lq, owner, 64);
        if (lane == 0) {
            const float lm = pick < nc ? (x[pick] - mx) - logf(sx) : -INFINITY;
            const long o = L.out_counter ? ((*L.out_counter % L.out_rows) + L.out_rows) % L.out_rows : 0;
            *reinterpret_cast<float2*>(L.logp + ((o * gridDim.x + n) * n_attr + a) * 2) = make_float2(lm, lq);
        }
    }
    return pick;
}

// MASKED = false is the plain draw of the three unmasked entry points (M unused).  MASKED = true: disallowed classes
// get -inf logits before the temperature, the max, the softmax and the nucleus, so the draw is over the renormalised
// allowed distribution; with every bit set it is bitwise the plain draw.
// LOGP: after the draw, write (lp_model, lp_sampler) of the drawn class (LogpArgs).  FORCED (implies LOGP): no draw, no
// RNG, no token write; the class is the target's.  lp_sampler = (v_c - m) - log(sum of e over the kept classes), -inf
// outside the mask or the nucleus kept set; lp_model = (x_c - mx) - log(sum exp(x - mx)) over the raw logits (its max
// and sum are the sampler's own when inv_t == 1 and no mask row applies).
// GRAMMAR: the row grammar (GrammarArgs) on top of the mask row, if any.  Drawing: every wave draws the bar-beat class
// first (the bar-beat wave keeps it, the others only learn the row's kind from it), then its own attribute under the
// kind's gram row.  FORCED: the kind is that of the target row's bar-beat class.
template <bool MASKED, bool LOGP = false, bool FORCED = false, bool GRAMMAR = false>
__global__ __launch_bounds__(64 * CWLT_MAX_ATTR) void sample_categorical_kernel(
    const float* __restrict__ logits, long ld, SampleArgs A, int n_attr, uint64_t seed,
    const int64_t* __restrict__ counter, int64_t* __restrict__ tokens, int64_t* __restrict__ song, long song_rows,
    int slot_keyed, const int64_t* __restrict__ row_key, const int64_t* __restrict__ row_step, MaskArgs M,
    LogpArgs L, GrammarArgs G) {
    static_assert(LOGP || !FORCED, "FORCED writes log-probs");
    __shared__ float e_s[CWLT_MAX_ATTR][256];
    const int lane = threadIdx.x & 63, a = threadIdx.x >> 6, n = blockIdx.x;
    if (a >= n_attr) return;                         // wave-uniform; no workgroup barriers in this kernel
    long forced = 0;
    if constexpr (FORCED) {
        forced = L.targets[(long)n * n_attr + a];
        if (forced < 0) return;                      // padding row: wave-uniform, nothing written
    }
    if constexpr (!GRAMMAR) {
        draw_attr<MASKED, LOGP, FORCED, false>(logits, ld, A, n_attr, seed, counter, tokens, song, song_rows, slot_keyed,
                                               row_key, row_step, M, L, G, e_s[a], n, lane, a, forced, true, KIND_NONE);
    } else if constexpr (FORCED) {
        int kind = KIND_POSITION;
        if (a != G.bar_attr) {
            const long tb = L.targets[(long)n * n_attr + G.bar_attr];
            kind = tb >= 0 && tb < A.n[G.bar_attr] ? grammar_kind(G.order[tb]) : KIND_NONE;
        }
        draw_attr<MASKED, LOGP, true, true>(logits, ld, A, n_attr, seed, counter, tokens, song, song_rows, slot_keyed,
                                            row_key, row_step, M, L, G, e_s[a], n, lane, a, forced, true, kind);
    } else {
        // every wave runs this call, on the same inputs: the same class in all of them
        const bool own = a == G.bar_attr;
        const int bb = draw_attr<MASKED, LOGP, false, true>(logits, ld, A, n_attr, seed, counter, tokens, song, song_rows,
                                                            slot_keyed, row_key, row_step, M, L, G, e_s[a], n, lane,
                                                            G.bar_attr, 0, own, KIND_POSITION);
        if (own) return;                             // wave-uniform
        __builtin_amdgcn_wave_barrier();             // the LDS row is reused: reads above stay before the writes below
        draw_attr<MASKED, LOGP, false, true>(logits, ld, A, n_attr, seed, counter, tokens, song, song_rows, slot_keyed,
                                             row_key, row_step, M, L, G, e_s[a], n, lane, a, 0, true,
                                             grammar_kind(G.order[bb]));
    }
}

}  // namespace cwlt

template <bool MASKED, bool LOGP, bool FORCED, bool GRAMMAR>
static void launch_sample(int64_t rows, int n_attr, void* stream, const float* logits, int64_t ld,
                          const cwlt::SampleArgs& A, uint64_t seed, const int64_t* counter, int64_t* tokens,
                          int64_t* song, int64_t song_rows, int slot_keyed, const int64_t* row_key,
                          const int64_t* row_step, const cwlt::MaskArgs& M, const cwlt::LogpArgs& L,
                          const cwlt::GrammarArgs& G) {
    hipLaunchKernelGGL((cwlt::sample_categorical_kernel<MASKED, LOGP, FORCED, GRAMMAR>), dim3((unsigned)rows),
                       dim3(64 * n_attr), 0, (hipStream_t)stream, logits, (long)ld, A, n_attr, seed, counter, tokens,
                       song, (long)song_rows, slot_keyed, row_key, row_step, M, L, G);
}

// lp: the log-prob output (LOGP instantiations); forced: score lp->targets instead of drawing (FORCED); gr: the row
// grammar (GRAMMAR), n_order its order entries.
static int sample(const float* logits, const int* n_class, const float* temperature, const float* top_p, int n_attr,
                  int64_t rows, int64_t ld, uint64_t seed, const int64_t* counter, int64_t* tokens, int64_t* song,
                  int64_t song_rows, int slot_keyed, void* stream, const int64_t* row_key = nullptr,
                  const int64_t* row_step = nullptr, const cwlt::MaskArgs* mask = nullptr,
                  const cwlt::LogpArgs* lp = nullptr, bool forced = false, const cwlt::GrammarArgs* gr = nullptr,
                  int n_order = 0) {
    using namespace cwlt;
    if (!logits || (!tokens && !forced) || rows <= 0) return CWLT_ERR_ARG;
    SampleArgs A;
    int width = 0;
    if (sample_args(n_class, temperature, top_p, n_attr, ld, &A, &width)) return CWLT_ERR_ARG;
    if (mask && table_words(mask->words, width)) return CWLT_ERR_ARG;
    if (gr && grammar_args(*gr, n_order, n_class, n_attr, width)) return CWLT_ERR_ARG;
    const MaskArgs M = mask ? *mask : MaskArgs{};
    const LogpArgs L = lp ? *lp : LogpArgs{};
    const GrammarArgs G = gr ? *gr : GrammarArgs{};
#define CWLT_SAMPLE_LAUNCH(MK, LP, FC, GR)                                                                            \
    launch_sample<MK, LP, FC, GR>(rows, n_attr, stream, logits, ld, A, seed, counter, tokens, song, song_rows,        \
                                  slot_keyed, row_key, row_step, M, L, G)
#define CWLT_SAMPLE_FORM(LP, FC)                                                                                      \
    do {                                                                                                              \
        if (gr) {                                                                                                     \
            if (mask) CWLT_SAMPLE_LAUNCH(true, LP, FC, true);                                                         \
            else CWLT_SAMPLE_LAUNCH(false, LP, FC, true);                                                             \
        } else {                                                                                                      \
            if (mask) CWLT_SAMPLE_LAUNCH(true, LP, FC, false);                                                        \
            else CWLT_SAMPLE_LAUNCH(false, LP, FC, false);                                                            \
        }                                                                                                             \
    } while (0)
    if (!lp)
        CWLT_SAMPLE_FORM(false, false);
    else if (!forced)
        CWLT_SAMPLE_FORM(true, false);
    else
        CWLT_SAMPLE_FORM(true, true);
#undef CWLT_SAMPLE_FORM
#undef CWLT_SAMPLE_LAUNCH
    return (int)hipGetLastError();
}

extern "C" int cwlt_sample_categorical(const float* logits, const int* n_class, const float* temperature,
                                       const float* top_p, int n_attr, int64_t rows, int64_t ld, uint64_t seed, const int64_t* counter,
                                       int64_t* tokens, int64_t* song, int64_t song_rows, void* stream) {
    return sample(logits, n_class, temperature, top_p, n_attr, rows, ld, seed, counter, tokens, song, song_rows, 0,
                  stream);
}

extern "C" int cwlt_sample_categorical_slots(const float* logits, const int* n_class, const float* temperature,
                                             const float* top_p, int n_attr, int64_t rows, int64_t ld, uint64_t seed,
                                             const int64_t* counter, int64_t* tokens, int64_t* song,
                                             int64_t song_rows, void* stream) {
    if (rows > (1L << 20)) return CWLT_ERR_ARG;             // row << 40 stays clear of the attribute factor
    return sample(logits, n_class, temperature, top_p, n_attr, rows, ld, seed, counter, tokens, song, song_rows, 1,
                  stream);
}

extern "C" int cwlt_sample_categorical_keyed(const float* logits, const int* n_class, const float* temperature,
                                             const float* top_p, int n_attr, int64_t rows, int64_t ld, uint64_t seed,
                                             const int64_t* key, const int64_t* step, int64_t* tokens, void* stream) {
    if (!key || !step || rows > (1L << 20)) return CWLT_ERR_ARG;
    return sample(logits, n_class, temperature, top_p, n_attr, rows, ld, seed, nullptr, tokens, nullptr, 0, 1, stream,
                  key, step);
}

extern "C" int cwlt_sample_categorical_masked(const float* logits, const int* n_class, const float* temperature,
                                              const float* top_p, int n_attr, int64_t rows, int64_t ld, uint64_t seed,
                                              const int64_t* counter, const int64_t* key, const int64_t* step,
                                              const int64_t* bar, const int64_t* sched, int64_t n_sched,
                                              const uint32_t* masks, int64_t mask_rows, int mask_words,
                                              int64_t* tokens, void* stream) {
    using namespace cwlt;
    if (rows > (1L << 20)) return CWLT_ERR_ARG;
    if (!key != !step || (!key && !counter)) return CWLT_ERR_ARG;    // keyed per row, or by slot and counter
    MaskArgs M{};
    bool masked = false;                             // this entry needs the table
    if (mask_args(bar, sched, n_sched, masks, mask_rows, mask_words, &M, &masked) || !masked) return CWLT_ERR_ARG;
    return sample(logits, n_class, temperature, top_p, n_attr, rows, ld, seed, key ? nullptr : counter, tokens, nullptr,
                  0, 1, stream, key, step, &M);
}

extern "C" int cwlt_sample_categorical_logp(const float* logits, const int* n_class, const float* temperature,
                                            const float* top_p, int n_attr, int64_t rows, int64_t ld, uint64_t seed,
                                            const int64_t* counter, const int64_t* key, const int64_t* step,
                                            const int64_t* bar, const int64_t* sched, int64_t n_sched,
                                            const uint32_t* masks, int64_t mask_rows, int mask_words,
                                            int64_t* tokens, float* logp, const int64_t* out_counter,
                                            int64_t out_rows, void* stream) {
    using namespace cwlt;
    if (!logp || rows > (1L << 20) || out_rows < 1 || (out_counter == nullptr && out_rows != 1)) return CWLT_ERR_ARG;
    if (!key != !step || (!key && !counter)) return CWLT_ERR_ARG;    // keyed per row, or by slot and counter
    MaskArgs M{};
    bool masked = false;
    if (mask_args(bar, sched, n_sched, masks, mask_rows, mask_words, &M, &masked)) return CWLT_ERR_ARG;
    const LogpArgs L{logp, out_counter, (long)out_rows, nullptr};
    return sample(logits, n_class, temperature, top_p, n_attr, rows, ld, seed, key ? nullptr : counter, tokens, nullptr,
                  0, 1, stream, key, step, masked ? &M : nullptr, &L);
}

extern "C" int cwlt_score_categorical(const float* logits, const int* n_class, const float* temperature,
                                      const float* top_p, int n_attr, int64_t rows, int64_t ld, const int64_t* targets,
                                      const int64_t* key, const int64_t* bar, const int64_t* sched, int64_t n_sched,
                                      const uint32_t* masks, int64_t mask_rows, int mask_words, float* logp,
                                      void* stream) {
    using namespace cwlt;
    if (!logp || !targets || rows > (1L << 20)) return CWLT_ERR_ARG;
    MaskArgs M{};
    bool masked = false;
    if (mask_args(bar, sched, n_sched, masks, mask_rows, mask_words, &M, &masked)) return CWLT_ERR_ARG;
    const LogpArgs L{logp, nullptr, 1, targets};
    return sample(logits, n_class, temperature, top_p, n_attr, rows, ld, 0, nullptr, nullptr, nullptr, 0, 1, stream,
                  key, nullptr, masked ? &M : nullptr, &L, true);
}

extern "C" int cwlt_sample_categorical_grammar(const float* logits, const int* n_class, const float* temperature,
                                               const float* top_p, int n_attr, int64_t rows, int64_t ld, uint64_t seed,
                                               const int64_t* counter, const int64_t* key, const int64_t* step,
                                               const int64_t* bar, const int64_t* sched, int64_t n_sched,
                                               const uint32_t* masks, int64_t mask_rows, int mask_words,
                                               const int64_t* beat, const int* order, int n_order,
                                               const uint32_t* gram, int gram_words, int bar_attr, int64_t* tokens,
                                               float* logp, const int64_t* out_counter, int64_t out_rows,
                                               void* stream) {
    using namespace cwlt;
    if (rows > (1L << 20)) return CWLT_ERR_ARG;
    if (!key != !step || (!key && !counter)) return CWLT_ERR_ARG;    // keyed per row, or by slot and counter
    if (logp && (out_rows < 1 || (out_counter == nullptr && out_rows != 1))) return CWLT_ERR_ARG;
    MaskArgs M{};
    bool masked = false;
    if (mask_args(bar, sched, n_sched, masks, mask_rows, mask_words, &M, &masked)) return CWLT_ERR_ARG;
    const GrammarArgs G{beat, order, gram, gram_words, bar_attr};   // checked by sample()
    const LogpArgs L{logp, out_counter, (long)out_rows, nullptr};
    return sample(logits, n_class, temperature, top_p, n_attr, rows, ld, seed, key ? nullptr : counter, tokens, nullptr,
                  0, 1, stream, key, step, masked ? &M : nullptr, logp ? &L : nullptr, false, &G, n_order);
}

extern "C" int cwlt_score_categorical_grammar(const float* logits, const int* n_class, const float* temperature,
                                              const float* top_p, int n_attr, int64_t rows, int64_t ld,
                                              const int64_t* targets, const int64_t* key, const int64_t* bar,
                                              const int64_t* sched, int64_t n_sched, const uint32_t* masks,
                                              int64_t mask_rows, int mask_words, const int64_t* beat, const int* order,
                                              int n_order, const uint32_t* gram, int gram_words, int bar_attr,
                                              float* logp, void* stream) {
    using namespace cwlt;
    if (!logp || !targets || rows > (1L << 20)) return CWLT_ERR_ARG;
    MaskArgs M{};
    bool masked = false;
    if (mask_args(bar, sched, n_sched, masks, mask_rows, mask_words, &M, &masked)) return CWLT_ERR_ARG;
    const GrammarArgs G{beat, order, gram, gram_words, bar_attr};   // checked by sample()
    const LogpArgs L{logp, nullptr, 1, targets};
    return sample(logits, n_class, temperature, top_p, n_attr, rows, ld, 0, nullptr, nullptr, nullptr, 0, 1, stream,
                  key, nullptr, masked ? &M : nullptr, &L, true, &G, n_order);
}

namespace cwlt {

// Bar count of the batch loop's constrained mode, after each draw: bar[n] += 1 when row n's bar-beat class is a Bar.
__global__ __launch_bounds__(256) void count_bars_kernel(const int64_t* __restrict__ tokens, long rows, int n_attr,
                                                         int bar_attr, const int* __restrict__ bar_mask,
                                                         int bar_classes, int64_t* __restrict__ bar) {
    const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= rows) return;
    const int64_t tk = tokens[n * n_attr + bar_attr];
    if (tk >= 0 && tk < bar_classes && bar_mask[tk]) bar[n] += 1;
}

// Position in the bar of the row grammar, after each draw: a row flagged fresh whose slot holds a song starts from
// that song's beat0; any other row moves by its drawn bar-beat class (Bar: -1, Beat_k: k, anything else: unchanged).
__global__ __launch_bounds__(256) void grammar_track_kernel(const int64_t* __restrict__ tokens, long rows, int n_attr,
                                                            int bar_attr, const int* __restrict__ order, int n_order,
                                                            const int64_t* __restrict__ fresh,
                                                            const int64_t* __restrict__ song,
                                                            const int64_t* __restrict__ beat0, long n_songs,
                                                            int64_t* __restrict__ beat) {
    const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= rows) return;
    if (fresh && fresh[n] != 0 && song[n] >= 0) {
        if (song[n] < n_songs) beat[n] = beat0[song[n]];
        return;
    }
    const int64_t tk = tokens[n * n_attr + bar_attr];
    if (tk < 0 || tk >= n_order) return;
    const int o = order[tk];
    if (o == -1 || o >= 0) beat[n] = o;
}

}  // namespace cwlt

extern "C" int cwlt_count_bars(const int64_t* tokens, int64_t rows, int n_attr, int bar_attr, const int* bar_mask,
                               int bar_classes, int64_t* bar, void* stream) {
    using namespace cwlt;
    if (!tokens || !bar_mask || !bar) return CWLT_ERR_ARG;
    if (rows < 1 || rows > (1L << 20) || n_attr < 1 || n_attr > CWLT_MAX_ATTR || bar_attr < 0 || bar_attr >= n_attr ||
        bar_classes < 1)
        return CWLT_ERR_ARG;
    hipLaunchKernelGGL(count_bars_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       tokens, (long)rows, n_attr, bar_attr, bar_mask, bar_classes, bar);
    return (int)hipGetLastError();
}

extern "C" int cwlt_grammar_track(const int64_t* tokens, int64_t rows, int n_attr, int bar_attr, const int* order,
                                  int n_order, const int64_t* fresh, const int64_t* song, const int64_t* beat0,
                                  int64_t n_songs, int64_t* beat, void* stream) {
    using namespace cwlt;
    if (!tokens || !order || !beat) return CWLT_ERR_ARG;
    if (rows < 1 || rows > (1L << 20) || n_attr < 1 || n_attr > CWLT_MAX_ATTR || bar_attr < 0 || bar_attr >= n_attr ||
        n_order < 1)
        return CWLT_ERR_ARG;
    if ((fresh || song || beat0) && (!fresh || !song || !beat0 || n_songs < 1)) return CWLT_ERR_ARG;   // all or none
    hipLaunchKernelGGL(grammar_track_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       tokens, (long)rows, n_attr, bar_attr, order, n_order, fresh, song, beat0, (long)n_songs, beat);
    return (int)hipGetLastError();
}
