// Prompt prefill: the f32 chunked causal-linear-attention forward with the recurrent state carried in and out.
//
// A prompt of P tokens leaves every (sequence, head) of the recurrent form (csrc/recurrent.hip) in the closed-form state
//   S = S0 + sum_t phi(k_t) (x) v_t ,  Z = Z0 + sum_t phi(k_t)
// and its attention rows are
//   out_l = phi(q_l) . (S0 + sum_{j<=l} phi(k_j) (x) v_j) / (phi(q_l) . (Z0 + sum_{j<=l} phi(k_j)) + eps),
// i.e. exactly what P calls of cwlt_recurrent_cla_step compute, up to the order of the f32 sums.  Used by
// generation.DecodeSession.prefill to feed a whole prompt per layer in one pass instead of one token per call.
//
// Layout: q, k, v, out in the projection GEMM's own (N, L, H, 64) row layout (row stride ld*), as
// cwlt_causal_linear_fwd; S (N, H, 64, 64) key-feature-major (S[n,h,d,m]) and Z (N, H, 64), the recurrent step's own
// state buffers, read at the start and overwritten with the state after the sequence's last valid token.
//
// Algorithm: the forward scan of cla.hip (chunk = 32 tokens, one workgroup of 2 waves per (n, h), wave w owns value
// columns [32w, 32w+32), the 64x64 running state in v_mfma_f32_32x32x2_f32 accumulators for the whole sequence),
// started from (S0, Z0) instead of zero and stopped after ceil(len / 32) chunks.  Rows at or past the sequence's
// length are masked in their FEATURES (phi(0) = 1, so a zero raw k row would still count) and never read from memory.
//
// Few streams (one song at the repo dims is 8 workgroups on 256 CUs): the segmented form cuts every sequence into runs
// of whole chunks, one workgroup each -- pass 1 reduces each run to its state increment, pass 2 turns the increments
// into starting states (S0, Z0 added), pass 3 is the scan above from each run's own start.
//
// Packed form (cwlt_causal_linear_fwd_state_packed): prompts of different lengths laid end to end in
// (R, H, 64) row buffers with a device table of song starts; the same scan kernel instantiated with the table in place
// of (lengths, L), one workgroup per (song, head), never segmented -- every song bit for bit the rectangular scan of it.
#include "cwlt_common.h"

namespace cwlt {
namespace prefill {

constexpr int D = 64;    // head dim
constexpr int C = 32;    // tokens per chunk
constexpr int LDT = 65;  // LDS row stride of the 32x64 operand tiles (odd: row- and column-type reads conflict-free)
constexpr int LDA = 33;  // LDS row stride of the 32x32 intra-chunk score tiles

__device__ __forceinline__ float phi(float x) { return x > 0.f ? x + 1.f : (expf(x) - 1.f) + 1.f; }

// accumulator register r of lane-half hf -> row of the 32x32 tile (column = lane & 31)
__device__ __forceinline__ constexpr int acc_row(int r, int hf) { return (r & 3) + 8 * (r >> 2) + 4 * hf; }

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}

// X[i][j] = sum_e a_t[i][e] * b_t[j][e]   (both tiles row-major 32x64, stride LDT) -> 32 MFMAs
__device__ __forceinline__ f32x16 prod_rows(const float* a_t, const float* b_t, int l31, int hf) {
    f32x16 acc = zero16();
#pragma unroll 8
    for (int s = 0; s < 32; ++s) acc = mfma(a_t[l31 * LDT + 2 * s + hf], b_t[l31 * LDT + 2 * s + hf], acc);
    return acc;
}

// acc[i][n] += sum_j x[i][j] * t[j][col0+n]   (x: 32x32 stride LDA) -> 16 MFMAs
__device__ __forceinline__ f32x16 prod_x_t(f32x16 acc, const float* x, const float* t, int col0, int l31, int hf) {
#pragma unroll 8
    for (int s = 0; s < 16; ++s) acc = mfma(x[l31 * LDA + 2 * s + hf], t[(2 * s + hf) * LDT + col0 + l31], acc);
    return acc;
}

// acc[i][n] += sum_{k in k0..k0+31} a_t[i][k] * S[k][n], S held in accumulator layout (rows on registers)
__device__ __forceinline__ f32x16 prod_state(f32x16 acc, const float* a_t, int k0, const f32x16& S, int l31, int hf) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc = mfma(a_t[l31 * LDT + k0 + acc_row(r, hf)], S[r], acc);
    return acc;
}

// S0[p][n] += sum_j a_t[j][p] * b_t[j][col0+n],  S1[p][n] += sum_j a_t[j][32+p] * b_t[j][col0+n]  -> 32 MFMAs
__device__ __forceinline__ void update_state(f32x16& S0, f32x16& S1, const float* a_t, const float* b_t, int col0,
                                             int l31, int hf) {
#pragma unroll 8
    for (int s = 0; s < 16; ++s) {
        const float b = b_t[(2 * s + hf) * LDT + col0 + l31];
        S0 = mfma(a_t[(2 * s + hf) * LDT + l31], b, S0);
        S1 = mfma(a_t[(2 * s + hf) * LDT + 32 + l31], b, S1);
    }
}

__device__ __forceinline__ void write4(float* t, int row, int col, float4 x) {
    float* p = t + row * LDT + col;
    p[0] = x.x; p[1] = x.y; p[2] = x.z; p[3] = x.w;
}
__device__ __forceinline__ float4 phi4(float4 x, bool valid) {
    if (!valid) return make_float4(0.f, 0.f, 0.f, 0.f);
    return make_float4(phi(x.x), phi(x.y), phi(x.z), phi(x.w));
}

// Chunks of one sequence a segment owns: [c0, c1), c1 <= the sequence's own chunk count nch.
__device__ __forceinline__ void seg_range(const int* lengths, int n, int L, int g, int cps, int& len, int& nch,
                                          int& c0, int& c1) {
    len = lengths ? lengths[n] : L;
    len = len < 0 ? 0 : (len > L ? L : len);
    nch = (len + C - 1) / C;
    c0 = g * cps;
    c1 = c0 + cps < nch ? c0 + cps : nch;
}

// Segmented form, pass 1: the state increment of each segment, sum over its rows of phi(k) (x) v and phi(k)
// (zero for a segment past its sequence's length) -> ws[(n*H + h)*G + g] = [dS (64 x 64, [d][m]) | dZ (64)].
__global__ __launch_bounds__(128) void cla_state_delta_kernel(const float* __restrict__ k, const float* __restrict__ v,
                                                              float* __restrict__ ws, const int* __restrict__ lengths,
                                                              int H, int L, int G, int cps, long ldk, long ldv) {
    __shared__ float ks[C * LDT];
    __shared__ float vs[C * LDT];
    const int nh = blockIdx.x / G, g = blockIdx.x % G, n = nh / H, h = nh % H;
    int len, nch, c0, c1;
    seg_range(lengths, n, L, g, cps, len, nch, c0, c1);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hf = lane >> 5;
    const float* kb = k + ((long)n * L) * ldk + h * D;
    const float* vb = v + ((long)n * L) * ldv + h * D;
    const int srow = tid >> 4, scol = (tid & 15) * 4;
    const float4 f4z = make_float4(0.f, 0.f, 0.f, 0.f);
    f32x16 S0 = zero16(), S1 = zero16();
    float zsum = 0.f;                                   // thread tid < 64: column tid of the key-feature sum
    for (int c = c0; c < c1; ++c) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int row = srow + 8 * it;
            const bool ok = (long)c * C + row < len;
            write4(ks, row, scol, phi4(ok ? load4(kb + ((long)c * C + row) * ldk + scol) : f4z, ok));
            write4(vs, row, scol, ok ? load4(vb + ((long)c * C + row) * ldv + scol) : f4z);
        }
        __syncthreads();
        update_state(S0, S1, ks, vs, 32 * w, l31, hf);
        if (tid < D) {
#pragma unroll 8
            for (int j = 0; j < C; ++j) zsum += ks[j * LDT + tid];
        }
        __syncthreads();
    }
    float* wb = ws + (long)blockIdx.x * (D * D + D);
    float* Sb = wb + 32 * w + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        Sb[acc_row(r, hf) * D] = S0[r];
        Sb[(32 + acc_row(r, hf)) * D] = S1[r];
    }
    if (tid < D) wb[D * D + tid] = zsum;
}

// Segmented form, pass 2: increments -> starting states, in place: ws[g] = (S, Z) + sum_{g' < g} ws[g'].
__global__ __launch_bounds__(256) void cla_state_prefix_kernel(const float* __restrict__ S, const float* __restrict__ Z,
                                                               float* __restrict__ ws, int G) {
    const int nh = blockIdx.x;
    float* wb = ws + (long)nh * G * (D * D + D);
    for (int e = threadIdx.x; e < D * D + D; e += blockDim.x) {
        float run = e < D * D ? S[(long)nh * D * D + e] : Z[(long)nh * D + e - D * D];
        for (int g0 = 0; g0 < G; g0 += 8) {  // 8 independent loads in flight, then the serial sum
            float d[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = g0 + j < G ? wb[(long)(g0 + j) * (D * D + D) + e] : 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (g0 + j < G) wb[(long)(g0 + j) * (D * D + D) + e] = run;
                run += d[j];
            }
        }
    }
}

// The scan proper.  G == 1: one workgroup per (n, h) starts from (S, Z) and writes the final state back.  G > 1:
// workgroup (n, h, g) runs segment g's chunks from the starting state pass 2 left in ws; the segment holding the
// sequence's last chunk writes the final state (no workgroup reads S or Z then, so in place is safe).
// PACKED: `seq` is the offset table cu (cwlt_common.h, seq_span) in place of L; workgroup (s, h) owns rows [cu[s],
// cu[s + 1]) of (R, H, 64) row buffers and runs all of the song's chunks from its row 0, never segmented (ws and
// lengths are NULL, G is 1) -- the rectangular scan of that song alone, chunk for chunk.
template <bool PACKED>
__global__ __launch_bounds__(128) void cla_fwd_state_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                            const float* __restrict__ v, float* __restrict__ o,
                                                            float* __restrict__ S, float* __restrict__ Z,
                                                            const float* __restrict__ ws, const int* __restrict__ lengths,
                                                            int H, typename SeqArg<PACKED>::type seq, int G_, int cps,
                                                            long ldq, long ldk, long ldv, long ldo, float eps) {
    __shared__ float qs[C * LDT];
    __shared__ float ks[C * LDT];
    __shared__ float vs[C * LDT];
    __shared__ float as[2][C * LDA];
    __shared__ float ksum[2][D];
    __shared__ float zs[2][C];

    const int G = PACKED ? 1 : G_;
    const int nh = blockIdx.x / G, g = blockIdx.x % G, n = nh / H, h = nh % H;
    int len, nch, c0, c1;
    long row0;  // the stream's first row
    if constexpr (PACKED) {
        seq_span<true>(seq, n, row0, len);
        nch = (len + C - 1) / C;
        c0 = 0;
        c1 = nch;
    } else {
        row0 = (long)n * seq;
        seg_range(lengths, n, seq, g, cps, len, nch, c0, c1);
    }
    if (c0 >= c1) return;  // nothing to add (a length of 0 leaves S and Z bit-for-bit as they are)

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hf = lane >> 5;
    const float* qb = q + row0 * ldq + h * D;
    const float* kb = k + row0 * ldk + h * D;
    const float* vb = v + row0 * ldv + h * D;
    float* ob = o + row0 * ldo + h * D;
    float* Sb = S + (long)nh * (D * D) + 32 * w + l31;  // this lane's value column m = 32w + l31
    float* Zb = Z + (long)nh * D;
    const float* Sin = G == 1 ? Sb : ws + (long)blockIdx.x * (D * D + D) + 32 * w + l31;
    const float* Zin = G == 1 ? Zb : ws + (long)blockIdx.x * (D * D + D) + D * D;

    const int srow = tid >> 4, scol = (tid & 15) * 4;
    const float4 f4z = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 rq[4], rk[4], rv[4];

#define CLA_STATE_LOAD(c)                                       \
    _Pragma("unroll") for (int it = 0; it < 4; ++it) {          \
        const long row = (long)(c) * C + srow + 8 * it;         \
        const bool ok = row < len;                              \
        rq[it] = ok ? load4(qb + row * ldq + scol) : f4z;       \
        rk[it] = ok ? load4(kb + row * ldk + scol) : f4z;       \
        rv[it] = ok ? load4(vb + row * ldv + scol) : f4z;       \
    }

    CLA_STATE_LOAD(c0);
    // starting state: S[d][m] for d in [0, 32) (S0) and [32, 64) (S1), in accumulator layout; Z into the key sum
    f32x16 S0, S1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        S0[r] = Sin[acc_row(r, hf) * D];
        S1[r] = Sin[(32 + acc_row(r, hf)) * D];
    }
    if (tid < D) ksum[0][tid] = Zin[tid];

    for (int c = c0; c < c1; ++c) {
        const int cb = (c - c0) & 1;  // key-sum buffer of this chunk
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int row = srow + 8 * it;
            const bool ok = c * C + row < len;
            write4(qs, row, scol, phi4(rq[it], ok));
            write4(ks, row, scol, phi4(rk[it], ok));
            write4(vs, row, scol, rv[it]);
        }
        __syncthreads();
        if (c + 1 < c1) { CLA_STATE_LOAD(c + 1); }

        // intra-chunk scores A = qf kf^T, causal-masked
        f32x16 A = prod_rows(qs, ks, l31, hf);
        float* aw = as[w];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = acc_row(r, hf);
            aw[i * LDA + l31] = (l31 <= i) ? A[r] : 0.f;
        }
        __builtin_amdgcn_wave_barrier();

        // normaliser: rowsum(A) + qf . ksum_prev (ksum_prev includes Z0)
        float den = 0.f;
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) den += aw[l31 * LDA + hf * 16 + jj];
        const float* kp = ksum[cb];
#pragma unroll 8
        for (int e = 0; e < 32; ++e) den = fmaf(qs[l31 * LDT + hf * 32 + e], kp[hf * 32 + e], den);
        den += __shfl_xor(den, 32, 64);
        if (hf == 0) zs[w][l31] = 1.0f / (den + eps);
        // running key sum for the next chunk (wave w owns e in [32w, 32w+32))
        {
            float ksn = 0.f;
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) ksn += ks[(hf * 16 + jj) * LDT + 32 * w + l31];
            ksn += __shfl_xor(ksn, 32, 64);
            if (hf == 0) ksum[cb ^ 1][32 * w + l31] = kp[32 * w + l31] + ksn;
        }
        __builtin_amdgcn_wave_barrier();

        // numerator: A v + qf S_prev
        f32x16 O = zero16();
        O = prod_x_t(O, aw, vs, 32 * w, l31, hf);
        O = prod_state(O, qs, 0, S0, l31, hf);
        O = prod_state(O, qs, 32, S1, l31, hf);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = acc_row(r, hf);
            const long row = (long)c * C + i;
            if (row < len) ob[row * ldo + 32 * w + l31] = O[r] * zs[w][i];
        }
        // state: S += kf^T v
        update_state(S0, S1, ks, vs, 32 * w, l31, hf);
        __syncthreads();
    }
#undef CLA_STATE_LOAD
    if (c1 != nch) return;  // not the sequence's last segment

#pragma unroll
    for (int r = 0; r < 16; ++r) {
        Sb[acc_row(r, hf) * D] = S0[r];
        Sb[(32 + acc_row(r, hf)) * D] = S1[r];
    }
    if (tid < D) Zb[tid] = ksum[(c1 - c0) & 1][tid];
}

}  // namespace prefill
}  // namespace cwlt

extern "C" {

int cwlt_prefill_segments(int N, int H, int L) {
    const int chunks = (L + cwlt::prefill::C - 1) / cwlt::prefill::C;
    if (N <= 0 || H <= 0 || chunks <= 1 || N * H >= 128) return 1;
    int G = (256 + N * H - 1) / (N * H);
    G = G < chunks ? G : chunks;
    const int cps = (chunks + G - 1) / G;
    return (chunks + cps - 1) / cps;  // every segment owns at least one chunk
}

int64_t cwlt_prefill_seg_floats(int N, int H, int segments) {
    return segments > 1 ? (int64_t)N * H * segments * (64 * 64 + 64) : 0;
}

/* Both forms.  cu == nullptr: N sequences of L rows.  cu != nullptr: the packed one -- N = n_songs, and the forward below
 * passes no lengths, L = 0, one segment and no workspace. */
static int fwd_state(const void* q, const void* k, const void* v, void* out, float* S, float* Z, const int* lengths,
                     int N, int H, int L, const int* cu, int head_dim, long ldq, long ldk, long ldv, long ldo, float eps,
                     int segments, float* seg_ws, int dtype, hipStream_t st) {
    using namespace cwlt::prefill;
    if (!q || !k || !v || !out || !S || !Z || N < 0 || H <= 0 || L < 0 || head_dim != 64) return CWLT_ERR_ARG;
    if (dtype != CWLT_F32) return CWLT_ERR_DTYPE;
    if (ldq % 4 || ldk % 4 || ldv % 4 || ldq < H * 64 || ldk < H * 64 || ldv < H * 64 || ldo < H * 64 ||
        ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16)   // 16-byte row loads of q, k, v
        return CWLT_ERR_ARG;
    if (cu && (int64_t)N * H > 0x7fffffffLL) return CWLT_ERR_ARG;
    if (segments < 1 || (segments > 1 && !seg_ws)) return CWLT_ERR_ARG;
    const int chunks = (L + C - 1) / C, cps = (chunks + segments - 1) / segments;
    if (chunks > 0 && (segments - 1) * cps >= chunks) return CWLT_ERR_ARG;  // every segment must own a chunk
    if (N == 0 || (!cu && L == 0)) return CWLT_OK;
    if (segments > 1) {
        hipLaunchKernelGGL(cla_state_delta_kernel, dim3(N * H * segments), dim3(128), 0, st, (const float*)k,
                           (const float*)v, seg_ws, lengths, H, L, segments, cps, ldk, ldv);
        hipLaunchKernelGGL(cla_state_prefix_kernel, dim3(N * H), dim3(256), 0, st, (const float*)S, (const float*)Z,
                           seg_ws, segments);
    }
    auto go = [&](auto kernel, auto seq) {   // seq: L or cu
        hipLaunchKernelGGL(kernel, dim3(N * H * segments), dim3(128), 0, st, (const float*)q, (const float*)k,
                           (const float*)v, (float*)out, S, Z, (const float*)seg_ws, lengths, H, seq, segments, cps,
                           ldq, ldk, ldv, ldo, eps);
    };
    cu ? go(cla_fwd_state_kernel<true>, cu) : go(cla_fwd_state_kernel<false>, L);
    return (int)hipGetLastError();
}

int cwlt_causal_linear_fwd_state(const void* q, const void* k, const void* v, void* out, float* S, float* Z,
                                 const int* lengths, int N, int H, int L, int head_dim, int64_t ldq, int64_t ldk,
                                 int64_t ldv, int64_t ldo, float eps, int segments, float* seg_ws, int dtype,
                                 void* stream) {
    return fwd_state(q, k, v, out, S, Z, lengths, N, H, L, nullptr, head_dim, ldq, ldk, ldv, ldo, eps, segments, seg_ws,
                     dtype, (hipStream_t)stream);
}

int cwlt_causal_linear_fwd_state_packed(const void* q, const void* k, const void* v, void* out, float* S, float* Z,
                                        const int* cu, int n_songs, int H, int head_dim, int64_t ldq, int64_t ldk,
                                        int64_t ldv, int64_t ldo, float eps, int dtype, void* stream) {
    if (!cu) return CWLT_ERR_ARG;   // to fwd_state a null table would mean the rectangular form
    return fwd_state(q, k, v, out, S, Z, nullptr, n_songs, H, 0, cu, head_dim, ldq, ldk, ldv, ldo, eps, 1, nullptr,
                     dtype, (hipStream_t)stream);
}

}  // extern "C"
