// Blending a policy with a reference model at sampling time (generation.generate_batch / generate_stream /
// score_songs / policy_stats with reference= and alpha=): with x the model's logits of one attribute and
// r the reference's, out = alpha x + (1 - alpha) r, so that softmax(out) is pi^alpha pi_ref^(1 - alpha) renormalised.
// The result is an ordinary logits row: every sampler, scorer and stats entry reads it as it reads a model's own.
// alpha is a device table with one row per song (or one shared row) and one entry per attribute; a row whose key is
// outside the table -- an idle (-1) or waiting (-2) stream slot -- is copied from `logits`.
// Arithmetic per element: b = 1 - alpha once in f32, then alpha x + b r (two products and a sum, contracted to an fma
// or not): alpha = 1 gives x and alpha = 0 gives r exactly for finite inputs (a -0 may come back +0).
#include "cwlt_common.h"

#define CWLT_MAX_ATTR 8

namespace cwlt {

struct BlendAttr {
    int n_attr;
    int end[CWLT_MAX_ATTR];                          // end[a]: one past the last column of attribute a
};

// One element: the attribute of column c picks its alpha.  end[] never decreases and is `width` from the last attribute
// on, so the count of ends at or below c is the attribute's index.
__device__ inline float blend_one(const BlendAttr& at, const float* __restrict__ al, int c, float x, float r) {
    int a = 0;
#pragma unroll
    for (int q = 0; q < CWLT_MAX_ATTR - 1; ++q) a += c >= at.end[q] ? 1 : 0;
    const float w = al[a], b = 1.0f - w;
    return w * x + b * r;
}

// One thread per V consecutive columns of one row (V = 4: one 16-byte access per operand; V = 1: the scalar form for
// bases or strides that do not allow it).  An attribute boundary may fall inside a vector, so alpha is chosen per
// element; a vector that reaches past `width` (the last one of a row) goes element by element and neither reads nor
// writes a column at or past width.  Each element is read, then written, by the same thread: out may be logits.
// rows * groups <= 2^20 * 2048 = 2^31 fits the unsigned index.
template <int V>
__global__ __launch_bounds__(256) void blend_kernel(const float* logits, long ld, const float* __restrict__ ref,
                                                    long ref_ld, BlendAttr at, int width,
                                                    const float* __restrict__ alpha, long n_alpha,
                                                    const int64_t* __restrict__ key, float* out, long ld_out,
                                                    unsigned rows) {
    const unsigned groups = (unsigned)(width + V - 1) / V, total = rows * groups;
    const unsigned stride = gridDim.x * blockDim.x;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const unsigned n = i / groups;
        const int c0 = (int)(i - n * groups) * V;
        long k = 0;
        if (n_alpha > 1) k = key ? key[n] : (long)n;
        const bool copy = k < 0 || k >= n_alpha;     // an idle or waiting slot: the row of logits as it is
        const float* x = logits + (long)n * ld + c0;
        const float* r = ref + (long)n * ref_ld + c0;
        float* o = out + (long)n * ld_out + c0;
        const float* al = alpha + (copy ? 0 : k) * at.n_attr;
        if (V == 4 && c0 + 4 <= width) {
            float4 v = *reinterpret_cast<const float4*>(x);
            if (!copy) {
                const float4 r4 = *reinterpret_cast<const float4*>(r);
                v.x = blend_one(at, al, c0, v.x, r4.x);
                v.y = blend_one(at, al, c0 + 1, v.y, r4.y);
                v.z = blend_one(at, al, c0 + 2, v.z, r4.z);
                v.w = blend_one(at, al, c0 + 3, v.w, r4.w);
            }
            *reinterpret_cast<float4*>(o) = v;
        } else {
#pragma unroll 1                                     // one vector per row at most: kept a loop, and out of the vector path
            for (int j = 0; j < V; ++j)
                if (c0 + j < width) o[j] = copy ? x[j] : blend_one(at, al, c0 + j, x[j], r[j]);
        }
    }
}

}  // namespace cwlt

extern "C" int cwlt_blend_logits(const float* logits, int64_t ld, const float* ref_logits, int64_t ref_ld,
                                 const int* n_class, int n_attr, const float* alpha, int64_t n_alpha,
                                 const int64_t* key, float* out, int64_t ld_out, int64_t rows, void* stream) {
    using namespace cwlt;
    if (!logits || !ref_logits || !alpha || !out || !n_class) return CWLT_ERR_ARG;
    if (n_attr < 1 || n_attr > CWLT_MAX_ATTR || n_alpha < 1 || rows < 1 || rows > (1L << 20)) return CWLT_ERR_ARG;
    if (out == ref_logits) return CWLT_ERR_ARG;
    BlendAttr at;
    at.n_attr = n_attr;
    int width = 0;
    for (int a = 0; a < CWLT_MAX_ATTR; ++a) {
        if (a < n_attr) {
            if (n_class[a] < 1 || n_class[a] > 256) return CWLT_ERR_ARG;
            width += n_class[a];
        }
        at.end[a] = width;
    }
    if (ld < width || ref_ld < width || ld_out < width) return CWLT_ERR_ARG;
    const bool vec = (((uintptr_t)logits | (uintptr_t)ref_logits | (uintptr_t)out) % 16) == 0 &&
                     ((ld | ref_ld | ld_out) % 4) == 0;
    const long groups = vec ? (width + 3) / 4 : width;
    long blocks = (rows * groups + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (vec)
        hipLaunchKernelGGL(blend_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, logits,
                           (long)ld, ref_logits, (long)ref_ld, at, width, alpha, (long)n_alpha, key, out, (long)ld_out,
                           (unsigned)rows);
    else
        hipLaunchKernelGGL(blend_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, logits,
                           (long)ld, ref_logits, (long)ref_ld, at, width, alpha, (long)n_alpha, key, out, (long)ld_out,
                           (unsigned)rows);
    return (int)hipGetLastError();
}
