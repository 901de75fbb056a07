// The device sampler's support rule, the one copy of it: which classes of an attribute a row may draw (constraint mask
// row, position rule, gram row) and which of them the nucleus keeps.  csrc/sample.hip draws and scores under it,
// csrc/policy_stats.hip takes entropies and KLs of the distribution it leaves.  Also the argument
// structs both kernels take, and the host-side checks of the tables behind them.
//
// How the device helpers take and return their values is part of the sampler's code generation, because the compiler
// simplifies each helper on its own before it inlines it (profiles/sampler_support_share.txt): they compute in local
// arrays and return a struct by value; flags go in as scalars, never through a pointer the helper cannot see behind; the
// callers read the returned flags in place; the attribute's offset is loaded before the rule's branches, not inside
// them.  Out-parameters by reference spill in the sampler's LOGP grammar forms (HISTORY §14).
#pragma once
#include "cwlt_common.h"

#define CWLT_MAX_ATTR 8

namespace cwlt {

struct SampleArgs {
    int n[CWLT_MAX_ATTR];
    int off[CWLT_MAX_ATTR];
    float inv_t[CWLT_MAX_ATTR];                      // 1 / temperature per attribute
    float top_p[CWLT_MAX_ATTR];                      // nucleus mass per attribute; >= 1: plain categorical
};

// Allowed-class table of the masked draw (cwlt_sample_categorical_masked): the song of row n is k (row_key[n], or n
// when slot-keyed by the counter); its mask row is sched[2k] + min(bar[n] - 1, sched[2k + 1] - 1), `words` uint32 per
// row, class c of attribute a allowed when bit off[a] + c is set.  k < 0 (idle / waiting slots), k >= n_sched, a
// schedule of length 0 and a row outside [0, rows) all draw unmasked.
struct MaskArgs {
    const int64_t* bar;
    const int64_t* sched;
    const uint32_t* masks;
    long n_sched, rows;
    int words;
};

// Row grammar of the GRAMMAR instantiations (the sampler kernel's last argument, after its LogpArgs, so every other
// argument keeps its offset).  beat[n]: where row n's song stands in its bar: -1 after a Bar row, k
// after Beat_k.  order[c] for each class c of attribute bar_attr: -2 the neutral class (a note row), -1 a Bar class,
// k >= 0 Beat_k, -3 never allowed.  c is allowed when order[c] == -1, or order[c] > beat[n] >= -1 with order[c] >= 0,
// or order[c] == -2 with beat[n] >= 0.  gram: 3 x words uint32 in the bit layout of MaskArgs::masks, row 0 what a NOTE
// row may carry in each attribute, row 1 a BAR row, row 2 a BEAT row.
struct GrammarArgs {
    const int64_t* beat;
    const int* order;
    const uint32_t* gram;
    int words;
    int bar_attr;
};

constexpr int KIND_NONE = -1;                        // an ill-formed forced target: nothing is allowed
constexpr int KIND_POSITION = 3;                     // the bar-beat attribute itself: the position rule, no gram row

__device__ __forceinline__ int grammar_kind(int o) { return o == -2 ? 0 : o == -1 ? 1 : o >= 0 ? 2 : KIND_NONE; }

// ok: the classes 4 * lane .. 4 * lane + 3 of the attribute the row may draw; row_masked: a mask row applies; cut
// (per lane): the grammar removes a class of this attribute.  alignas: a struct of 8 bytes or less is returned packed
// into one integer, and the sampler then unpacks ok with shifts; a larger one comes back field by field.
// After any change to this struct or to how the helpers below pass their values, rerun tools/isa_compare.py on
// sample.hip and policy_stats.hip against the commit before: nothing else re-checks the sampler's code.
struct alignas(16) AllowedClasses {
    bool ok[4];
    bool row_masked, cut;
};

// The classes of attribute a (lane-blocked: lane l owns classes 4l .. 4l + 3) that row n may draw.  MASKED: the mask
// row of the row's song, row_key[n] or n.  GRAMMAR, on top of it: kind KIND_POSITION for the bar-beat attribute, else
// the gram row, KIND_NONE = no class.
template <bool MASKED, bool GRAMMAR>
__device__ __forceinline__ AllowedClasses allowed_classes(const SampleArgs& A, const MaskArgs& M, const GrammarArgs& G,
                                                          const int64_t* row_key, int n, int lane, int a,
                                                          int kind) {
    const int nc = A.n[a], off = A.off[a];
    bool ok[4] = {true, true, true, true};
    bool row_masked = false, cut = false;
    if constexpr (MASKED) {
        const long k = row_key ? row_key[n] : (long)n;
        if (k >= 0 && k < M.n_sched) {
            const long first = M.sched[2 * k], len = M.sched[2 * k + 1];
            long b = M.bar[n] - 1;
            b = b < 0 ? 0 : b < len - 1 ? b : len - 1;
            const long row = first + b;
            if (len > 0 && row >= 0 && row < M.rows) {
                row_masked = true;
                const uint32_t* w = M.masks + row * M.words;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int bit = off + lane * 4 + j;         // < sum n_class <= 32 * words: inside the row
                    ok[j] = lane * 4 + j < nc ? ((w[bit >> 5] >> (bit & 31)) & 1u) != 0 : false;
                }
            }
        }
    }
    if constexpr (GRAMMAR) {
        if (kind == KIND_POSITION) {
            const long bt = G.beat[n];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = lane * 4 + j;
                if (c < nc) {
                    const int o = G.order[c];        // order holds >= nc entries (checked by the entry points)
                    const bool g = o == -1 || (o >= 0 && o > bt) || (o == -2 && bt >= 0);
                    cut = cut || !g;
                    ok[j] = ok[j] && g;
                }
            }
        } else {
            const uint32_t* w = G.gram + (kind < 0 ? 0 : kind) * G.words;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int bit = off + lane * 4 + j;             // < sum n_class <= 32 * words: inside the row
                if (lane * 4 + j < nc) {
                    const bool g = kind >= 0 && ((w[bit >> 5] >> (bit & 31)) & 1u) != 0;
                    cut = cut || !g;
                    ok[j] = ok[j] && g;
                }
            }
        }
    }
    return {{ok[0], ok[1], ok[2], ok[3]}, row_masked, cut};
}

// The distribution the sampler draws attribute a from: v the tempered logits (-inf outside the allowed classes), m
// their max, e = exp(v - m) on the allowed classes inside the nucleus and 0 elsewhere.  keep: the allowed classes, and
// tot_all: 0 -- with KEEP, on a nucleus row: keep the classes inside the nucleus too, tot_all the sum of e before its
// cut.
struct SamplerSupport {
    float v[4], e[4];
    bool keep[4];
    float m, tot_all;
};

// ok0 .. ok3: AllowedClasses::ok of the lane, as scalars (see the head of this file).  `ew`: the wave's LDS row (>= nc
// floats), written and read by the nucleus ranking; a caller that uses one row twice puts a wave barrier between the
// calls.
template <bool KEEP>
__device__ __forceinline__ SamplerSupport sampler_support(const float* x, const SampleArgs& A, int a, int nc, int lane,
                                                          bool ok0, bool ok1, bool ok2, bool ok3, float* ew) {
    const bool ok[4] = {ok0, ok1, ok2, ok3};
    float v[4];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane * 4 + j;
        v[j] = c < nc && ok[j] ? x[c] * A.inv_t[a] : -INFINITY;
        m = fmaxf(m, v[j]);
    }
    m = wave_max(m);
    float e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = lane * 4 + j < nc && ok[j] ? expf(v[j] - m) : 0.f;
    bool keep[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) keep[j] = lane * 4 + j < nc && ok[j];
    float tot_all = 0.f;
    if (A.top_p[a] < 1.0f) {
        // nucleus (dqn_policy/model.py:33-47): in descending-probability order keep every class whose PRECEDING
        // mass is <= p (the class that crosses p is kept); probabilities there are exp/(sum + 1e-5).  The mass
        // ahead of class i needs no sort: G_i = sum of e_j over classes ranked before i (larger e, ties: larger
        // index first, as argsort()[::-1] orders them).  One broadcast LDS read per class, four running sums per lane.
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
        const float limit = A.top_p[a] * (tot * (1.0f + 1e-5f));
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = ahead[j] <= limit ? e[j] : 0.f;
        if constexpr (KEEP) {
#pragma unroll
            for (int j = 0; j < 4; ++j) keep[j] = keep[j] && ahead[j] <= limit;
            tot_all = tot;
        }
    }
    return {{v[0], v[1], v[2], v[3]}, {e[0], e[1], e[2], e[3]}, {keep[0], keep[1], keep[2], keep[3]}, m, tot_all};
}

// ---- host side: the checks every entry point makes before a launch; each returns 0 = ok, 1 = refused ----

// The attribute table: n_attr in 1 .. CWLT_MAX_ATTR, n_class in 1 .. 256, temperature > 0, top_p > 0 (NULL: 1), and a
// logits row of ld >= *width = sum n_class floats.
inline int sample_args(const int* n_class, const float* temperature, const float* top_p, int n_attr, int64_t ld,
                       SampleArgs* A, int* width) {
    if (!n_class || n_attr <= 0 || n_attr > CWLT_MAX_ATTR) return 1;
    int off = 0;
    for (int a = 0; a < n_attr; ++a) {
        if (n_class[a] <= 0 || n_class[a] > 256) return 1;
        if (temperature && !(temperature[a] > 0.f)) return 1;
        A->n[a] = n_class[a];
        A->off[a] = off;
        A->inv_t[a] = temperature ? 1.0f / temperature[a] : 1.0f;
        A->top_p[a] = top_p ? top_p[a] : 1.0f;
        if (!(A->top_p[a] > 0.f)) return 1;
        off += n_class[a];
    }
    *width = off;
    return ld < off;
}

// The constraint table: all three pointers, or none (*masked = false: unmasked).  That a row holds the attributes'
// classes is checked where their number is known (table_words).
inline int mask_args(const int64_t* bar, const int64_t* sched, int64_t n_sched, const uint32_t* masks,
                     int64_t mask_rows, int mask_words, MaskArgs* M, bool* masked) {
    *masked = bar || sched || masks;
    if (!*masked) return 0;
    if (!bar || !sched || !masks || n_sched < 1 || mask_rows < 1 || mask_words < 1) return 1;
    *M = MaskArgs{bar, sched, masks, (long)n_sched, (long)mask_rows, mask_words};
    return 0;
}

// A mask or gram row of `words` uint32 holds a bit for each of the `width` classes.
inline int table_words(int words, int width) { return (int64_t)words * 32 < width; }

// The row grammar's tables: all of them, bar_attr an attribute, an order entry for each of its classes.
inline int grammar_args(const GrammarArgs& G, int n_order, const int* n_class, int n_attr, int width) {
    if (!G.beat || !G.order || !G.gram || G.words < 1 || G.bar_attr < 0 || G.bar_attr >= n_attr) return 1;
    return n_order < n_class[G.bar_attr] || table_words(G.words, width);
}

}  // namespace cwlt
