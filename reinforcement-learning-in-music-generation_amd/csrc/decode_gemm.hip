// Row-batched decode step: one CW token for each of M songs, the projections as skinny f32 GEMMs on MFMA.
//
// cwlt_decode_step (decode.hip) runs every projection as a GEMV with one grid row per song, so each song streams all
// 156 MB of f32 weights per token and N songs cost N times the weight traffic.  Here a workgroup owns a tile of
// MT = 64 songs x 64*NB output columns, so a token step reads each weight once per 64 songs:
//
//   out[m, :] = epilogue(W . prologue(x[m, :]) + bias)       (same contract as decode_gemv_kernel)
//
//   * prologue: LayerNorm (optionally followed by a second one) of each row, by ln_rows_kernel: one wave per row,
//     the same in-register reduction as the GEMV's prologue, the normalised row stored to x_out (or to the caller's
//     scratch) where the GEMM reads it;
//   * GEMM: v_mfma_f32_16x16x4_f32, exact f32 in and out (no bf16 cast of the weights).  A = x rows (songs), B = W^T.
//     Per 16-deep k step a lane loads one float4 of each of its 4 x row blocks and NB weight row blocks (lane l holds
//     row l & 15, k = k0 + 4(l >> 4) .. +3), and MFMA t in 0..3 takes component t: the k order of the f32 fma chain is
//     a fixed permutation of 0..K-1.  The next step's loads are issued before the current step's MFMAs;
//   * split-K: S slices of K, S chosen from (n_out, K) only; each slice writes its partial tile to the caller's scratch
//     and finalize_kernel sums them in slice order, then bias, exact-erf GELU and the residual.  S = 1 applies the
//     epilogue in the GEMM itself.  No workgroup waits on another.
//
// Batch invariance (bitwise): an output element is a k-ordered fma chain over its own x row and weight row, the slice
// partials are added in a fixed order and the LayerNorm statistics are one wave's reduction of that row alone, all
// fixed by (n_out, K).  Rows past M load row M - 1 and are not stored.  So a song's result does not depend on M, on
// its position in a tile or on the other songs.
//
// cwlt_decode_step_rows enqueues the whole token step with these GEMMs, the same embedding gather and recurrent
// attention step as cwlt_decode_step, and the same per-song workspace layout (songs ws floats apart).
//
// Compiler report (-Rpass-analysis=kernel-resource-usage, gfx950): no scratch, no spills;
//   decode_gemm_kernel<1>: 50 VGPR, decode_gemm_kernel<2>: 60 VGPR, finalize_kernel: 8 VGPR,
//   ln_rows_kernel<1/2/5/8>: 20/24/42/64 VGPR (all 8 waves/SIMD).
// Issuing four k steps' loads ahead (a 4-deep register ring, 174/220 VGPR) measured slower: 210k vs 219k tokens/s at
// 256 songs, 306k vs 398k at 1024.
#include "cwlt.h"
#include "cwlt_common.h"

extern "C" int cwlt_recurrent_cla_step(const void* q, const void* k, const void* v, float* S, float* Z, void* out,
                                       int N, int H, int head_dim, int64_t ldq, int64_t ldk, int64_t ldv,
                                       int64_t ldo, float eps, int dtype, void* stream);
extern "C" int cwlt_cw_embed_fwd(const int64_t* tokens, const void* const* tables, const int* widths,
                                 const int* nrows, int n_attr, void* out, int64_t rows, int64_t ldo, int dtype,
                                 void* stream);

namespace cwlt {
namespace dgemm {

constexpr int MT = 64;          // songs per workgroup tile
constexpr int KS = 16;          // k per step: 4 MFMA 16x16x4
constexpr int MAX_M = 4096;     // songs per call
constexpr int MAX_N = 4096;     // output columns per call
constexpr int TARGET = 64;      // split-K aims at >= TARGET (n-tile, slice) pairs per 64-song tile

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

__device__ __forceinline__ float sum4(float4 v) { return (v.x + v.y) + (v.z + v.w); }

// LayerNorm of the K-vector held as NCH float4 per lane (invalid slots are zero and stay zero); the reduction of
// decode.hip's GEMV prologue, so the normalised rows are the same bits as the GEMV path's
template <int NCH>
__device__ __forceinline__ void ln_in_wave(float4 (&x)[NCH], const float* __restrict__ w, const float* __restrict__ b,
                                           int K4, int lane, float inv_k, float eps) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) s += sum4(x[c]);
    const float mean = wave_sum(s) * inv_k;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c * 64 + lane < K4) {
            const float dx = x[c].x - mean, dy = x[c].y - mean, dz = x[c].z - mean, dw = x[c].w - mean;
            q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
    }
    const float rstd = rsqrtf(wave_sum(q) * inv_k + eps);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int i = c * 64 + lane;
        if (i < K4) {
            const float4 g = ((const float4*)w)[i], o = ((const float4*)b)[i];
            x[c].x = (x[c].x - mean) * rstd * g.x + o.x;
            x[c].y = (x[c].y - mean) * rstd * g.y + o.y;
            x[c].z = (x[c].z - mean) * rstd * g.z + o.z;
            x[c].w = (x[c].w - mean) * rstd * g.w + o.w;
        }
    }
}

// xo[m, :] = LN2(LN1(x[m, :])) (LN2 optional); one wave per row, 4 rows per workgroup
template <int NCH>
__global__ __launch_bounds__(256) void ln_rows_kernel(const float* __restrict__ x, long ld_x,
                                                      const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                      const float* __restrict__ ln2_w, const float* __restrict__ ln2_b,
                                                      float eps, float* __restrict__ xo, long ld_xo, int M, int K) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;                            // wave-uniform; no barriers
    const int K4 = K >> 2;
    float4 v[NCH];
    const float4* xr = (const float4*)(x + (long)m * ld_x);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int i = c * 64 + lane;
        v[c] = i < K4 ? xr[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float inv_k = 1.0f / (float)K;
    ln_in_wave<NCH>(v, ln_w, ln_b, K4, lane, inv_k, eps);
    if (ln2_w) ln_in_wave<NCH>(v, ln2_w, ln2_b, K4, lane, inv_k, eps);
    float4* dst = (float4*)(xo + (long)m * ld_xo);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int i = c * 64 + lane;
        if (i < K4) dst[i] = v[c];
    }
}

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// One 64-song x 64*NB-column tile over k in [k_lo, k_hi) (a multiple of 16 wide).  grid (n tiles, m tiles, slices);
// 4 waves, wave w owns columns [n_tile + 16*NB*w, +16*NB).  part == NULL: epilogue, out[m*ld_out + n]; else the raw
// sum goes to part[(slice*M + m)*Nout + n].
template <int NB>
__global__ __launch_bounds__(256) void decode_gemm_kernel(
    const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ x, long ld_x,
    const float* __restrict__ res, long ld_res, float* __restrict__ out, long ld_out, float* __restrict__ part, int M,
    int Nout, int K, int kslice, int act) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int col = lane & 15, grp = lane >> 4;
    const int m0 = blockIdx.y * MT;
    const int n0 = blockIdx.x * (64 * NB) + wave * (16 * NB);
    if (n0 >= Nout) return;                        // wave-uniform; the kernel has no barriers
    const int k_lo = blockIdx.z * kslice;
    const int k_hi = min(K, k_lo + kslice);
    const float* xp[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) xp[b] = x + (long)min(m0 + b * 16 + col, M - 1) * ld_x + 4 * grp;
    const float* wp[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) wp[b] = W + (long)min(n0 + b * 16 + col, Nout - 1) * K + 4 * grp;

    f32x4 acc[4][NB];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    float4 xa[4], wa[NB];
#pragma unroll
    for (int b = 0; b < 4; ++b) xa[b] = load4(xp[b] + k_lo);
#pragma unroll
    for (int b = 0; b < NB; ++b) wa[b] = load4(wp[b] + k_lo);
    for (int k = k_lo; k < k_hi; k += KS) {
        const int kn = min(k + KS, k_hi - KS);     // the last step re-loads its own k: no guarded loads
        float4 xb[4], wb[NB];
#pragma unroll
        for (int b = 0; b < 4; ++b) xb[b] = load4(xp[b] + kn);
#pragma unroll
        for (int b = 0; b < NB; ++b) wb[b] = load4(wp[b] + kn);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                acc[i][j] = mfma(xa[i].x, wa[j].x, acc[i][j]);
                acc[i][j] = mfma(xa[i].y, wa[j].y, acc[i][j]);
                acc[i][j] = mfma(xa[i].z, wa[j].z, acc[i][j]);
                acc[i][j] = mfma(xa[i].w, wa[j].w, acc[i][j]);
            }
#pragma unroll
        for (int b = 0; b < 4; ++b) xa[b] = xb[b];
#pragma unroll
        for (int b = 0; b < NB; ++b) wa[b] = wb[b];
    }
    // D of 16x16x4: column = lane & 15 (output column n), row = 4 * (lane >> 4) + r (song)
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int n = n0 + j * 16 + col;
        if (n >= Nout) continue;
        const float bn = (part == nullptr && bias) ? bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + i * 16 + 4 * grp + r;
                if (m >= M) continue;
                float y = acc[i][j][r];
                if (part) {
                    part[((long)blockIdx.z * M + m) * Nout + n] = y;
                } else {
                    y += bn;
                    if (act == 1) y = gelu_erf(y);
                    if (res) y += res[(long)m * ld_res + n];
                    out[(long)m * ld_out + n] = y;
                }
            }
    }
}

// out[m, n] = epi(sum over slices s = 0..S-1, in order, of part[s, m, n] + bias[n]); grid (n blocks of 256, M)
__global__ __launch_bounds__(256) void finalize_kernel(const float* __restrict__ part, int S,
                                                       const float* __restrict__ bias, const float* __restrict__ res,
                                                       long ld_res, float* __restrict__ out, long ld_out, int M,
                                                       int Nout, int act) {
    const int n = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
    if (n >= Nout) return;
    const long MN = (long)M * Nout;
    const float* p = part + (long)m * Nout + n;
    float y = p[0];
    for (int s = 1; s < S; ++s) y += p[s * MN];
    if (bias) y += bias[n];
    if (act == 1) y = gelu_erf(y);
    if (res) y += res[(long)m * ld_res + n];
    out[(long)m * ld_out + n] = y;
}

struct Args {
    const float *W, *bias, *xin;
    long ld_x;
    const float *ln_w, *ln_b, *ln2_w, *ln2_b;
    float eps;
    const float* res;
    long ld_res;
    float* out;
    long ld_out;
    float* x_out;
    long ld_xo;
    int Nout, K, act;
};

static bool shape_ok(int Nout, int K) { return K >= KS && K <= 2048 && K % KS == 0 && Nout > 0 && Nout <= MAX_N; }

static int nb_of(int Nout) { return Nout >= 1024 ? 2 : 1; }

// split-K plan from (Nout, K) alone: slices of whole 16-deep steps, at least 4 steps each
struct Split {
    int S, kslice;
};
static Split split_of(int Nout, int K) {
    const int ntiles = (Nout + 64 * nb_of(Nout) - 1) / (64 * nb_of(Nout));
    const int steps = K / KS;
    int s = (TARGET + ntiles - 1) / ntiles;
    s = max(1, min(s, steps / 4));
    const int per = (steps + s - 1) / s;           // steps per slice
    return Split{(steps + per - 1) / per, per * KS};
}

// scratch floats of one call: the partial tiles, then the normalised rows (used when a prologue has no x_out)
static int64_t scratch_floats(int Nout, int K, int M) {
    const Split sp = split_of(Nout, K);
    return (sp.S > 1 ? (int64_t)sp.S * M * Nout : 0) + (int64_t)M * K;
}

template <int NCH>
static void launch_ln(const Args& a, float* xo, long ld_xo, int M, hipStream_t st) {
    hipLaunchKernelGGL((ln_rows_kernel<NCH>), dim3((M + 3) / 4), dim3(256), 0, st, a.xin, a.ld_x, a.ln_w, a.ln_b,
                       a.ln2_w, a.ln2_b, a.eps, xo, ld_xo, M, a.K);
}

// the GEMM with its prologue / split-K finalize; scratch: scratch_floats(Nout, K, M) floats (may be NULL when the
// call needs none: S == 1 and no prologue without x_out)
static int gemm(const Args& a, int M, float* scratch, hipStream_t st) {
    if (!shape_ok(a.Nout, a.K) || M <= 0 || M > MAX_M) return CWLT_ERR_ARG;
    const Split sp = split_of(a.Nout, a.K);
    const float* x = a.xin;
    long ld_x = a.ld_x;
    if (a.ln_w) {
        float* xo = a.x_out;
        long ld_xo = a.ld_xo;
        if (!xo) {
            if (!scratch) return CWLT_ERR_ARG;
            xo = scratch + (sp.S > 1 ? (int64_t)sp.S * M * a.Nout : 0);
            ld_xo = a.K;
        }
        const int nch = (a.K + 255) / 256;
        if (nch <= 1) launch_ln<1>(a, xo, ld_xo, M, st);
        else if (nch <= 2) launch_ln<2>(a, xo, ld_xo, M, st);
        else if (nch <= 5) launch_ln<5>(a, xo, ld_xo, M, st);
        else launch_ln<8>(a, xo, ld_xo, M, st);
        x = xo;
        ld_x = ld_xo;
    }
    float* part = nullptr;
    if (sp.S > 1) {
        if (!scratch) return CWLT_ERR_ARG;
        part = scratch;
    }
    const int nb = nb_of(a.Nout);
    const dim3 grid((a.Nout + 64 * nb - 1) / (64 * nb), (M + MT - 1) / MT, sp.S);
    if (nb == 2)
        hipLaunchKernelGGL((decode_gemm_kernel<2>), grid, dim3(256), 0, st, a.W, a.bias, x, ld_x, a.res, a.ld_res,
                           a.out, a.ld_out, part, M, a.Nout, a.K, sp.kslice, a.act);
    else
        hipLaunchKernelGGL((decode_gemm_kernel<1>), grid, dim3(256), 0, st, a.W, a.bias, x, ld_x, a.res, a.ld_res,
                           a.out, a.ld_out, part, M, a.Nout, a.K, sp.kslice, a.act);
    if (part) {
        hipLaunchKernelGGL(finalize_kernel, dim3((a.Nout + 255) / 256, M), dim3(256), 0, st, part, sp.S, a.bias,
                           a.res, a.ld_res, a.out, a.ld_out, M, a.Nout, a.act);
    }
    return (int)hipGetLastError();
}

static bool model_ok(const cwlt_decode_model* m) {
    return m && m->layers && m->tables && m->widths && m->nrows && m->w_in && m->w_heads && m->n_layer > 0 &&
           m->n_head > 0 && m->d_model == m->n_head * 64 && shape_ok(m->d_model, m->d_model) &&
           shape_ok(m->d_ff, m->d_model) && shape_ok(m->d_model, m->d_ff) && shape_ok(m->d_model, m->emb_width) &&
           shape_ok(3 * m->d_model, m->d_model) && shape_ok(m->n_logits, m->d_model) && m->n_attr > 0;
}

// per-song floats of the step's workspace: cwlt_decode_step's layout
static int64_t per_song(const cwlt_decode_model* m) { return (int64_t)m->emb_width + 9L * m->d_model + m->d_ff; }

// the largest scratch any of the step's GEMMs asks for (the normalised heads input is the hidden buffer or this)
static int64_t step_scratch(const cwlt_decode_model* m, int M) {
    const int D = m->d_model, F = m->d_ff;
    int64_t s = scratch_floats(D, m->emb_width, M);
    s = max(s, scratch_floats(3 * D, D, M));
    s = max(s, scratch_floats(D, D, M));
    s = max(s, scratch_floats(F, D, M));
    s = max(s, scratch_floats(D, F, M));
    s = max(s, scratch_floats(m->n_logits, D, M));
    return s;
}

}  // namespace dgemm
}  // namespace cwlt

extern "C" {

int64_t cwlt_decode_gemm_scratch_floats(int n_out, int K, int n_songs) {
    using namespace cwlt::dgemm;
    if (!shape_ok(n_out, K) || n_songs <= 0 || n_songs > MAX_M) return -1;
    return scratch_floats(n_out, K, n_songs);
}

int cwlt_decode_gemm(const float* W, const float* bias, const float* xin, const float* ln_w, const float* ln_b,
                     const float* ln2_w, const float* ln2_b, float eps, const float* res, float* out, float* x_out,
                     int n_out, int K, int act, int n_songs, int64_t ld_x, int64_t ld_res, int64_t ld_out,
                     int64_t ld_xo, float* scratch, void* stream) {
    using namespace cwlt::dgemm;
    if (!W || !xin || !out || n_songs <= 0 || n_songs > MAX_M || (act != 0 && act != 1) || (ln_w && !ln_b) ||
        (ln2_w && (!ln_w || !ln2_b)) || !shape_ok(n_out, K) || ld_x < K || (ld_x & 3) || ld_out < n_out ||
        (res && ld_res < n_out) || (x_out && ln_w && (ld_xo < K || (ld_xo & 3))))
        return CWLT_ERR_ARG;
    Args a{W, bias, xin, (long)ld_x, ln_w, ln_b, ln2_w, ln2_b, eps, res, (long)ld_res, out, (long)ld_out, x_out,
           (long)ld_xo, n_out, K, act};
    return gemm(a, n_songs, scratch, (hipStream_t)stream);
}

int64_t cwlt_decode_rows_workspace_floats(const cwlt_decode_model* m, int n_songs) {
    using namespace cwlt::dgemm;
    if (!model_ok(m) || n_songs <= 0 || n_songs > MAX_M) return -1;
    return (int64_t)n_songs * per_song(m) + step_scratch(m, n_songs);
}

int cwlt_decode_step_rows(const cwlt_decode_model* m, const int64_t* tokens, float* work, float* hidden, float* logits,
                          int n_songs, void* stream) {
    using namespace cwlt::dgemm;
    if (!model_ok(m) || !tokens || !work || !logits || n_songs <= 0 || n_songs > MAX_M) return CWLT_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int D = m->d_model, F = m->d_ff, E = m->emb_width, M = n_songs;
    const long ws = (long)per_song(m);
    float* emb = work;
    float* x0 = emb + E;
    float* xn = x0 + D;
    float* qkv = xn + D;
    float* att = qkv + 3 * D;
    float* s1 = att + D;
    float* x1 = s1 + D;
    float* hh = x1 + D;
    float* s2 = hh + F;
    float* scratch = work + (int64_t)M * ws;       // after the songs' rows
    int rc = cwlt_cw_embed_fwd(tokens, m->tables, m->widths, m->nrows, m->n_attr, emb, M, ws, CWLT_F32, stream);
    if (rc) return rc;
    // x0 = in_linear(emb) + pe[0]
    {
        Args a{m->w_in, m->b_in, emb, ws, nullptr, nullptr, nullptr, nullptr, 0.f, m->pe0, 0, x0, ws, nullptr, 0, D, E,
               0};
        if ((rc = gemm(a, M, scratch, st))) return rc;
    }
    for (int l = 0; l < m->n_layer; ++l) {
        const cwlt_decode_layer& L = m->layers[l];
        if (!L.wqkv || !L.wo || !L.w1 || !L.w2 || !L.ln1_w || !L.ln1_b || !L.ln2_w || !L.ln2_b || !L.S || !L.Z)
            return CWLT_ERR_ARG;
        const float* x = l == 0 ? x0 : xn;         // layer input (normalised by the previous layer's norm2)
        {
            const cwlt_decode_layer* P = l ? &m->layers[l - 1] : nullptr;
            Args a{L.wqkv, L.bqkv, l ? s2 : x0, ws, P ? P->ln2_w : nullptr, P ? P->ln2_b : nullptr, nullptr, nullptr,
                   m->eps_ln, nullptr, 0, qkv, ws, l ? xn : nullptr, ws, 3 * D, D, 0};
            if ((rc = gemm(a, M, scratch, st))) return rc;
        }
        rc = cwlt_recurrent_cla_step(qkv, qkv + D, qkv + 2 * D, L.S, L.Z, att, M, m->n_head, 64, ws, ws, ws, ws,
                                     m->eps_attn, CWLT_F32, stream);
        if (rc) return rc;
        {
            Args a{L.wo, L.bo, att, ws, nullptr, nullptr, nullptr, nullptr, 0.f, x, ws, s1, ws, nullptr, 0, D, D, 0};
            if ((rc = gemm(a, M, scratch, st))) return rc;
        }
        {
            Args a{L.w1, L.b1, s1, ws, L.ln1_w, L.ln1_b, nullptr, nullptr, m->eps_ln, nullptr, 0, hh, ws, x1, ws, F, D,
                   1};
            if ((rc = gemm(a, M, scratch, st))) return rc;
        }
        {
            Args a{L.w2, L.b2, hh, ws, nullptr, nullptr, nullptr, nullptr, 0.f, x1, ws, s2, ws, nullptr, 0, D, F, 0};
            if ((rc = gemm(a, M, scratch, st))) return rc;
        }
    }
    // heads on norm(norm2_last(s2)); the normalised row is what forward_hidden returns
    {
        const cwlt_decode_layer& P = m->layers[m->n_layer - 1];
        Args a{m->w_heads, m->b_heads, s2, ws, P.ln2_w, P.ln2_b, m->lnf_w, m->lnf_w ? m->lnf_b : nullptr, m->eps_ln,
               nullptr, 0, logits, (long)m->n_logits, hidden, (long)D, m->n_logits, D, 0};
        if ((rc = gemm(a, M, scratch, st))) return rc;
    }
    return CWLT_OK;
}

}  // extern "C"
