// Soft preferences for generation (generation.Preference, `preferences=`): an additive bias per class and
// bar, and a repetition penalty by how often and how recently the song has carried a class.  Like the blend
// (blend.hip) these are row-wise kernels in front of the unchanged samplers: cwlt_prefer_logits writes ordinary logits,
//   out[n][c] = ((x[n][c] + b) - f * s) - (s > 0 ? p : 0),
// b the song's bias row for the row's bar count, s = seen[n][c], f / p the song's frequency / presence penalty for
// the attribute of c (0 for the attribute's class 0, the neutral class, and without `seen`).  `seen` is one f32 per
// class and song, moved after every row by seen = seen * decay + hit: cwlt_prefer_track (one row per slot, after a
// draw) and cwlt_prefer_scan / cwlt_prefer_scan_packed (every row of given songs, padded to one length or laid end to
// end, for the scorers) share seen_step.
// Every product and sum is rounded on its own in f32 (fp contract off in prefer_one and seen_step: v_mul_f32 +
// v_add_f32, no v_fmac_f32), so the device is bitwise the numpy float32 restatement (sampling.prefer_logits_f32,
// Preference.seen_states) and generation and scoring see the same state.
#include "cwlt_common.h"

#define CWLT_MAX_ATTR 8

namespace cwlt {

struct PreferAttr {
    int n_attr;
    int end[CWLT_MAX_ATTR];                          // end[a]: one past the last column of attribute a
};

// The attribute of column c and its first column.  end[] never decreases and is `width` from the last attribute on.
__device__ inline int attr_of(const PreferAttr& at, int c, int* first) {
    int a = 0;
#pragma unroll
    for (int q = 0; q < CWLT_MAX_ATTR - 1; ++q) a += c >= at.end[q] ? 1 : 0;
    *first = a > 0 ? at.end[a - 1] : 0;
    return a;
}

// The apply formula of one element, each operation rounded on its own.  pen: the song's {frequency[A], presence[A],
// decay} row, NULL without a `seen` (then s is 0 as well and only the bias is added).
__device__ inline float prefer_one(const PreferAttr& at, const float* __restrict__ pen, int c, float x, bool has_b,
                                   float b, float s) {
#pragma clang fp contract(off)
    int first;
    const int a = attr_of(at, c, &first);
    const bool on = pen != nullptr && c != first;    // class 0 of every attribute is never penalised
    const float f = on ? pen[a] : 0.0f, p = on ? pen[at.n_attr + a] : 0.0f;
    float v = x;
    if (has_b) v = v + b;
    const float fs = f * s;
    v = v - fs;
    v = v - (s > 0.0f ? p : 0.0f);
    return v;
}

// The recurrence of one element: the product, then the sum.
__device__ inline float seen_step(float s, float d, float h) {
#pragma clang fp contract(off)
    const float m = s * d;
    return m + h;
}

// 1 when row `tok` (n_attr ids) carries class c - first in the attribute of column c.
__device__ inline float hit_of(const PreferAttr& at, const int64_t* __restrict__ tok, int c) {
    int first;
    const int a = attr_of(at, c, &first);
    return tok[a] == (int64_t)(c - first) ? 1.0f : 0.0f;
}

// blend_kernel's layout: one thread per V consecutive columns of one row (V = 4: 16-byte accesses; V = 1: the scalar
// form), the attribute chosen per element, the last vector of a row element by element, no column at or past width
// touched; each element is read, then written, by one thread: out may be logits.  A row whose song is outside [0,
// n_songs) -- an idle or waiting stream slot -- is copied.
template <int V>
__global__ __launch_bounds__(256) void prefer_logits_kernel(const float* logits, long ld, PreferAttr at, int width,
                                                            const int64_t* __restrict__ key,
                                                            const int64_t* __restrict__ bar,
                                                            const int64_t* __restrict__ sched, long n_songs,
                                                            const float* __restrict__ bias, long bias_rows,
                                                            long ld_bias, const float* __restrict__ pen,
                                                            const float* __restrict__ seen, long ld_seen, float* out,
                                                            long ld_out, unsigned rows) {
    const unsigned groups = (unsigned)(width + V - 1) / V, total = rows * groups;
    const unsigned stride = gridDim.x * blockDim.x;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const unsigned n = i / groups;
        const int c0 = (int)(i - n * groups) * V;
        const long k = key ? key[n] : (long)n;
        const bool copy = k < 0 || k >= n_songs;
        const float* x = logits + (long)n * ld + c0;
        float* o = out + (long)n * ld_out + c0;
        const float* b = nullptr;
        if (!copy && sched && bias) {
            const long first = sched[2 * k], nr = sched[2 * k + 1];
            if (nr > 0) {
                long j = bar ? bar[n] - 1 : 0;
                j = j < 0 ? 0 : (j > nr - 1 ? nr - 1 : j);
                if (first >= 0 && first + j < bias_rows) b = bias + (first + j) * ld_bias + c0;
            }
        }
        const float* s = seen && !copy ? seen + (long)n * ld_seen + c0 : nullptr;
        const float* pn = s ? pen + k * (2 * at.n_attr + 1) : nullptr;
        if (V == 4 && c0 + 4 <= width) {
            float4 v = *reinterpret_cast<const float4*>(x);
            if (!copy) {
                float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f), s4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (b) b4 = *reinterpret_cast<const float4*>(b);
                if (s) s4 = *reinterpret_cast<const float4*>(s);
                v.x = prefer_one(at, pn, c0, v.x, b != nullptr, b4.x, s4.x);
                v.y = prefer_one(at, pn, c0 + 1, v.y, b != nullptr, b4.y, s4.y);
                v.z = prefer_one(at, pn, c0 + 2, v.z, b != nullptr, b4.z, s4.z);
                v.w = prefer_one(at, pn, c0 + 3, v.w, b != nullptr, b4.w, s4.w);
            }
            *reinterpret_cast<float4*>(o) = v;
        } else {
#pragma unroll 1
            for (int j = 0; j < V; ++j)
                if (c0 + j < width)
                    o[j] = copy ? x[j]
                                : prefer_one(at, pn, c0 + j, x[j], b != nullptr, b ? b[j] : 0.0f, s ? s[j] : 0.0f);
        }
    }
}

// One thread per (row, column).  A row flagged fresh whose slot holds a song starts from that song's seen0 (its drawn
// token belongs to the song that just ended); a row without a song is left alone; any other moves by its drawn token.
__global__ __launch_bounds__(256) void prefer_track_kernel(const int64_t* __restrict__ tokens, unsigned rows,
                                                           PreferAttr at, int width, const float* __restrict__ pen,
                                                           long n_songs, const int64_t* __restrict__ fresh,
                                                           const int64_t* __restrict__ song,
                                                           const float* __restrict__ seen0, float* __restrict__ seen,
                                                           long ld_seen) {
    const unsigned total = rows * (unsigned)width, stride = gridDim.x * blockDim.x;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const unsigned n = i / (unsigned)width;
        const int c = (int)(i - n * (unsigned)width);
        const long k = song ? song[n] : (long)n;
        if (k < 0 || k >= n_songs) continue;
        float* s = seen + (long)n * ld_seen + c;
        if (fresh && fresh[n] != 0) {
            *s = seen0[k * width + c];
            continue;
        }
        *s = seen_step(*s, pen[k * (2 * at.n_attr + 1) + 2 * at.n_attr], hit_of(at, tokens + (long)n * at.n_attr, c));
    }
}

// One thread per (song, column) walks the song's rows in order from a zero state and writes the state after rows
// 0 .. t into row t: threads of one song are neighbours in c, so every load and store is coalesced across columns.
// A song outside [0, n_songs) has decay 0: its rows hold the hit of their own token alone.
// PACKED: `seq` is the int32 offset table cu in place of Lb, song sg owns rows [cu[sg], cu[sg + 1]) (a thread's own
// two words: the songs of one wave differ).
template <bool PACKED>
__global__ __launch_bounds__(256) void prefer_scan_kernel(const int64_t* __restrict__ tokens, unsigned nb,
                                                          typename SeqArg<PACKED>::type seq, PreferAttr at, int width,
                                                          const float* __restrict__ pen, long n_songs,
                                                          const int64_t* __restrict__ key,
                                                          float* __restrict__ seen_rows, long ld) {
    const unsigned total = nb * (unsigned)width, stride = gridDim.x * blockDim.x;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const unsigned sg = i / (unsigned)width;
        const int c = (int)(i - sg * (unsigned)width);
        long row0, Lb;
        if constexpr (PACKED) {
            row0 = seq[sg];
            Lb = seq[sg + 1] - row0;
        } else {
            row0 = (long)sg * seq;
            Lb = seq;
        }
        const long k = key ? key[row0] : (long)sg;
        const float d = k < 0 || k >= n_songs ? 0.0f : pen[k * (2 * at.n_attr + 1) + 2 * at.n_attr];
        int first;
        const int a = attr_of(at, c, &first);
        const int64_t mine = (int64_t)(c - first);
        float s = 0.0f;
        for (long t = 0; t < Lb; ++t) {
            const long row = row0 + t;
            s = seen_step(s, d, tokens[row * at.n_attr + a] == mine ? 1.0f : 0.0f);
            seen_rows[row * ld + c] = s;
        }
    }
}

// The attribute table of the three entries -> width, or -1 for arguments they all refuse.
static int prefer_attr(const int* n_class, int n_attr, PreferAttr* at) {
    if (!n_class || n_attr < 1 || n_attr > CWLT_MAX_ATTR) return -1;
    at->n_attr = n_attr;
    int width = 0;
    for (int a = 0; a < CWLT_MAX_ATTR; ++a) {
        if (a < n_attr) {
            if (n_class[a] < 1 || n_class[a] > 256) return -1;
            width += n_class[a];
        }
        at->end[a] = width;
    }
    return width;
}

static unsigned prefer_blocks(long elements) {
    long blocks = (elements + 255) / 256;
    return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

}  // namespace cwlt

extern "C" int cwlt_prefer_logits(const float* logits, int64_t ld, const int* n_class, int n_attr, const int64_t* key,
                                  const int64_t* bar, const int64_t* sched, int64_t n_songs, const float* bias,
                                  int64_t bias_rows, int64_t ld_bias, const float* pen, const float* seen,
                                  int64_t ld_seen, float* out, int64_t ld_out, int64_t rows, void* stream) {
    using namespace cwlt;
    if (!logits || !out) return CWLT_ERR_ARG;
    PreferAttr at;
    const int width = prefer_attr(n_class, n_attr, &at);
    if (width < 0 || n_songs < 1 || rows < 1 || rows > (1L << 20)) return CWLT_ERR_ARG;
    if (ld < width || ld_out < width) return CWLT_ERR_ARG;
    if ((bias != nullptr) != (sched != nullptr) || bias_rows < 0 || (bias && (bias_rows < 1 || ld_bias < width)))
        return CWLT_ERR_ARG;
    if (seen && (!pen || ld_seen < width)) return CWLT_ERR_ARG;
    if (seen == out || bias == out) return CWLT_ERR_ARG;
    const bool vec = (((uintptr_t)logits | (uintptr_t)out | (uintptr_t)bias | (uintptr_t)seen) % 16) == 0 &&
                     ((ld | ld_out | (bias ? ld_bias : 0) | (seen ? ld_seen : 0)) % 4) == 0;
    const long groups = vec ? (width + 3) / 4 : width;
    const unsigned blocks = prefer_blocks(rows * groups);
    if (vec)
        hipLaunchKernelGGL(prefer_logits_kernel<4>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, (long)ld,
                           at, width, key, bar, sched, (long)n_songs, bias, (long)bias_rows, (long)ld_bias, pen, seen,
                           (long)ld_seen, out, (long)ld_out, (unsigned)rows);
    else
        hipLaunchKernelGGL(prefer_logits_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, (long)ld,
                           at, width, key, bar, sched, (long)n_songs, bias, (long)bias_rows, (long)ld_bias, pen, seen,
                           (long)ld_seen, out, (long)ld_out, (unsigned)rows);
    return (int)hipGetLastError();
}

extern "C" int cwlt_prefer_track(const int64_t* tokens, int64_t rows, const int* n_class, int n_attr,
                                 const float* pen, int64_t n_songs, const int64_t* fresh, const int64_t* song,
                                 const float* seen0, float* seen, int64_t ld_seen, void* stream) {
    using namespace cwlt;
    if (!tokens || !pen || !seen) return CWLT_ERR_ARG;
    PreferAttr at;
    const int width = prefer_attr(n_class, n_attr, &at);
    if (width < 0 || n_songs < 1 || rows < 1 || rows > (1L << 20) || ld_seen < width) return CWLT_ERR_ARG;
    if ((fresh || song || seen0) && (!fresh || !song || !seen0)) return CWLT_ERR_ARG;               // all or none
    hipLaunchKernelGGL(prefer_track_kernel, dim3(prefer_blocks(rows * width)), dim3(256), 0, (hipStream_t)stream,
                       tokens, (unsigned)rows, at, width, pen, (long)n_songs, fresh, song, seen0, seen, (long)ld_seen);
    return (int)hipGetLastError();
}

extern "C" int cwlt_prefer_scan(const int64_t* tokens, int64_t nb, int64_t Lb, const int* n_class, int n_attr,
                                const float* pen, int64_t n_songs, const int64_t* key, float* seen_rows, int64_t ld,
                                void* stream) {
    using namespace cwlt;
    if (!tokens || !pen || !seen_rows) return CWLT_ERR_ARG;
    PreferAttr at;
    const int width = prefer_attr(n_class, n_attr, &at);
    if (width < 0 || n_songs < 1 || nb < 1 || Lb < 1 || nb > (1L << 20) || Lb > (1L << 20) || nb * Lb > (1L << 20) ||
        ld < width)
        return CWLT_ERR_ARG;
    hipLaunchKernelGGL(prefer_scan_kernel<false>, dim3(prefer_blocks(nb * width)), dim3(256), 0, (hipStream_t)stream,
                       tokens, (unsigned)nb, (int)Lb, at, width, pen, (long)n_songs, key, seen_rows, (long)ld);
    return (int)hipGetLastError();
}

extern "C" int cwlt_prefer_scan_packed(const int64_t* tokens, const int* cu, int64_t n_block, const int* n_class,
                                       int n_attr, const float* pen, int64_t n_songs, const int64_t* key,
                                       float* seen_rows, int64_t ld, void* stream) {
    using namespace cwlt;
    if (!tokens || !cu || !pen || !seen_rows) return CWLT_ERR_ARG;
    PreferAttr at;
    const int width = prefer_attr(n_class, n_attr, &at);
    if (width < 0 || n_songs < 1 || n_block < 1 || n_block > (1L << 20) || ld < width) return CWLT_ERR_ARG;
    hipLaunchKernelGGL(prefer_scan_kernel<true>, dim3(prefer_blocks(n_block * width)), dim3(256), 0,
                       (hipStream_t)stream, tokens, (unsigned)n_block, cu, at, width, pen, (long)n_songs, key,
                       seen_rows, (long)ld);
    return (int)hipGetLastError();
}
