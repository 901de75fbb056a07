// Particle generation (generation.generate_particles): sequential Monte Carlo with the device sampler
// as the proposal.  K consecutive rows of a lock-step decode pool are the particles of one song.  Per token
//   cwlt_particle_weigh     adds the log of the draw's allowed mass, lp_model - lp_sampler summed over the attributes,
//                           to each live row's log-weight, counts the row and decides on the device whether it ended;
// every `resample_every` tokens
//   cwlt_particle_resample  one workgroup per song: effective sample size, systematic resampling into an ancestor
//                           vector, the evidence increment, the weights reset;
//   cwlt_particle_gather    dst[b][n] = src[b][anc[n]] for one family of per-row buffers, moved rows only -- the
//                           song-to-song copy of the decode state and of every small per-row state -- and, as the
//                           second phase of a move through scratch, dst[b][n] = src[b][n] for the same rows.
// None of the three synchronises with the host or allocates: weigh sits inside the captured token, the other two are
// enqueued between replays.  No cross-workgroup communication, no atomics; every barrier is workgroup-uniform.
#include "cwlt_common.h"

namespace cwlt {

// One thread per row.  The sums are plain f32 additions in attribute order (there is no product to contract into an
// fma): bitwise sampling.particle_weigh_f32.
__global__ __launch_bounds__(256) void particle_weigh_kernel(const float* __restrict__ logp,
                                                             const int64_t* __restrict__ out_counter, long out_rows,
                                                             long rows, int n_attr, const int64_t* __restrict__ bar,
                                                             long bar_cond, const int64_t* __restrict__ cap,
                                                             float* __restrict__ lw, int64_t* __restrict__ len,
                                                             int64_t* __restrict__ done) {
    const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= rows || done[n] != 0) return;
    const long o = out_counter ? (long)(*out_counter % out_rows) : 0;
    const float* p = logp + ((o * rows + n) * n_attr) * 2;
    float s = 0.f;
    for (int a = 0; a < n_attr; ++a) s = __fadd_rn(s, __fsub_rn(p[2 * a], p[2 * a + 1]));
    lw[n] = __fadd_rn(lw[n], s);
    const int64_t l = len[n] + 1;
    len[n] = l;
    done[n] = (bar[n] >= bar_cond || l >= cap[n]) ? 1 : 0;
}

constexpr uint64_t RESAMPLE_STREAM = 0x7061727469636c65ull;     // keeps u off the sampler's keys of the same seed

// One workgroup per group of K consecutive rows, one thread per row (blockDim = K rounded up to whole waves).
// The prefix sums are sequential per wave and over the wave totals, so the prefix array never decreases and the binary
// search below is the "first row whose prefix exceeds the threshold" of the restatement.
// KEYED (cwlt_particle_resample_keyed, the particle stream of DESIGN §4.6o): u is keyed by the group's song and the
// song's own event index, pos[g * pos_stride] / every - 1, not by the group's place and the run's event; a group
// without a song (or before its first event) is left alone, workgroup-uniformly and ahead of every barrier.  song, pos,
// pos_stride and every are KEYED's alone; everything after the key is the one body of both entries.
template <bool KEYED>
__global__ __launch_bounds__(1024) void particle_resample_kernel(float* __restrict__ lw,
                                                                 const int64_t* __restrict__ done, int K,
                                                                 float ess_frac, uint64_t seed, long event,
                                                                 const int64_t* __restrict__ song,
                                                                 const int64_t* __restrict__ pos, long pos_stride,
                                                                 long every, int64_t* __restrict__ anc,
                                                                 float* __restrict__ u_out,
                                                                 float* __restrict__ ess_out,
                                                                 int* __restrict__ resampled,
                                                                 float* __restrict__ log_z) {
    __shared__ float c_s[1024];                      // e, then its inclusive prefix
    __shared__ float red_s[3][16];                   // per wave: max, sum of e^2, total of e
    __shared__ int live_s[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n_wave = blockDim.x >> 6;
    const long g = blockIdx.x, row0 = g * K;
    long key = g;
    if (KEYED) {
        key = song[g];
        event = pos[g * pos_stride] / every - 1;
        if (key < 0 || event < 0) {                  // the same for the whole workgroup
            if (tid < K) anc[row0 + tid] = row0 + tid;
            if (tid == 0) {
                u_out[g] = 0.f;
                ess_out[g] = 0.f;
                resampled[g] = 0;
            }
            return;
        }
    }
    const bool own = tid < K;
    const float x = own ? lw[row0 + tid] : -INFINITY;
    const bool live = own && done[row0 + tid] == 0;
    const float wm = wave_max(x);
    const unsigned long long lm = __ballot(live);
    if (lane == 0) {
        red_s[0][w] = wm;
        live_s[w] = lm != 0ull;
    }
    __syncthreads();
    float m = -INFINITY;
    int any_live = 0;
    for (int q = 0; q < n_wave; ++q) {
        m = fmaxf(m, red_s[0][q]);
        any_live |= live_s[q];
    }
    const float e = own && m > -INFINITY ? expf(x - m) : 0.f;
    c_s[tid] = e;
    const float w2 = wave_sum(e * e);
    __syncthreads();
    if (lane == 0) {                                 // this wave's 64 entries, in order
        float run = 0.f;
        for (int i = w * 64; i < w * 64 + 64; ++i) {
            run += c_s[i];
            c_s[i] = run;
        }
        red_s[1][w] = w2;
        red_s[2][w] = run;
    }
    __syncthreads();
    float off = 0.f, s2 = 0.f;
    for (int q = 0; q < n_wave; ++q) {
        off += q < w ? red_s[2][q] : 0.f;
        s2 += red_s[1][q];
    }
    const float c = off + c_s[tid];                  // rows past K add 0: c of the last thread is the total
    __syncthreads();
    c_s[tid] = c;
    __syncthreads();
    const float s = c_s[K - 1];
    const float ess = s * s / s2;
    const uint32_t r = rng_pair(seed ^ RESAMPLE_STREAM, ((uint64_t)event << 32) + (uint64_t)key);
    const float u = (float)(r >> 8) * (1.0f / 16777216.0f);      // [0, 1)
    const bool keep = !any_live || !(s > 0.f) || ess >= ess_frac * (float)K;      // workgroup-uniform
    if (tid == 0) {
        u_out[g] = u;
        ess_out[g] = ess;
        resampled[g] = keep ? 0 : 1;
        if (!keep) log_z[g] = log_z[g] + (m + logf(s / (float)K));
    }
    if (!own) return;                                // no barrier below
    if (keep) {
        anc[row0 + tid] = row0 + tid;
        return;
    }
    const float t = ((float)tid + u) / (float)K * s;
    int lo = 0, hi = K - 1;                          // first i with c_s[i] > t, K - 1 when there is none
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c_s[mid] > t) hi = mid; else lo = mid + 1;
    }
    anc[row0 + tid] = row0 + lo;
    lw[row0 + tid] = 0.f;
}

// Work items are (row, block, slab of 4 x 256 units of V); the workgroups grid-stride over them and skip, workgroup-
// uniformly, the items of rows that do not move.  copy_back: the source row is n itself (the way back from scratch).
// All index arithmetic is 64-bit.
template <typename V>
__global__ __launch_bounds__(256) void particle_gather_kernel(char* __restrict__ dst, const char* __restrict__ src,
                                                              const int64_t* __restrict__ anc, long rows,
                                                              long row_bytes, long n_blocks, long block_stride,
                                                              long slabs, int copy_back) {
    const long units = row_bytes / (long)sizeof(V);
    const long per_row = n_blocks * slabs, items = rows * per_row;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const long n = item / per_row, rem = item - n * per_row;
        const long a = anc[n];
        if (a == n || a < 0 || a >= rows) continue;
        const long b = rem / slabs, c = rem - b * slabs;
        const V* s = reinterpret_cast<const V*>(src + b * block_stride + (copy_back ? n : a) * row_bytes);
        V* d = reinterpret_cast<V*>(dst + b * block_stride + n * row_bytes);
        const long first = c * 1024 + threadIdx.x;
        V v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (first + q * 256 < units) v[q] = s[first + q * 256];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (first + q * 256 < units) d[first + q * 256] = v[q];
    }
}

template <typename V>
static int launch_gather(void* dst, const void* src, const int64_t* anc, long rows, long row_bytes, long n_blocks,
                         long block_stride, int copy_back, hipStream_t st) {
    const long units = row_bytes / (long)sizeof(V), slabs = (units + 1023) / 1024;
    long blocks = rows * n_blocks * slabs;
    if (blocks > 2048) blocks = 2048;                // one resident set of 256-thread workgroups on 256 CUs
    hipLaunchKernelGGL(particle_gather_kernel<V>, dim3((unsigned)blocks), dim3(256), 0, st, (char*)dst,
                       (const char*)src, anc, rows, row_bytes, n_blocks, block_stride, slabs, copy_back);
    return (int)hipGetLastError();
}

}  // namespace cwlt

extern "C" int cwlt_particle_weigh(const float* logp, const int64_t* out_counter, int64_t out_rows, int64_t rows,
                                   int n_attr, const int64_t* bar, int64_t bar_cond, const int64_t* cap, float* lw,
                                   int64_t* len, int64_t* done, void* stream) {
    using namespace cwlt;
    if (!logp || !bar || !cap || !lw || !len || !done) return CWLT_ERR_ARG;
    if (rows < 1 || rows > (1L << 20) || n_attr < 1 || n_attr > 8 || out_rows < 1 || (!out_counter && out_rows != 1))
        return CWLT_ERR_ARG;
    hipLaunchKernelGGL(particle_weigh_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       logp, out_counter, (long)out_rows, (long)rows, n_attr, bar, (long)bar_cond, cap, lw, len, done);
    return (int)hipGetLastError();
}

extern "C" int cwlt_particle_resample(float* lw, const int64_t* done, int64_t groups, int particles, float ess_frac,
                                      uint64_t seed, int64_t event, int64_t* anc, float* u, float* ess,
                                      int* resampled, float* log_z, void* stream) {
    using namespace cwlt;
    if (!lw || !done || !anc || !u || !ess || !resampled || !log_z) return CWLT_ERR_ARG;
    if (particles < 2 || particles > 1024 || groups < 1 || groups * particles > (1L << 20) || event < 0 ||
        event > 0xffffffffL || !(ess_frac >= 0.f && ess_frac <= 1.f))
        return CWLT_ERR_ARG;
    const int threads = (particles + 63) / 64 * 64;
    hipLaunchKernelGGL(particle_resample_kernel<false>, dim3((unsigned)groups), dim3(threads), 0, (hipStream_t)stream,
                       lw, done, particles, ess_frac, seed, (long)event, nullptr, nullptr, 0L, 1L, anc, u, ess,
                       resampled, log_z);
    return (int)hipGetLastError();
}

extern "C" int cwlt_particle_resample_keyed(float* lw, const int64_t* done, int64_t groups, int particles,
                                            float ess_frac, uint64_t seed, const int64_t* song, const int64_t* pos,
                                            int64_t pos_stride, int64_t every, int64_t* anc, float* u, float* ess,
                                            int* resampled, float* log_z, void* stream) {
    using namespace cwlt;
    if (!lw || !done || !song || !pos || !anc || !u || !ess || !resampled || !log_z) return CWLT_ERR_ARG;
    if (particles < 2 || particles > 1024 || groups < 1 || groups * particles > (1L << 20) || pos_stride < 1 ||
        pos_stride > (1L << 20) || every < 1 || !(ess_frac >= 0.f && ess_frac <= 1.f))
        return CWLT_ERR_ARG;
    const int threads = (particles + 63) / 64 * 64;
    hipLaunchKernelGGL(particle_resample_kernel<true>, dim3((unsigned)groups), dim3(threads), 0, (hipStream_t)stream,
                       lw, done, particles, ess_frac, seed, 0L, song, pos, (long)pos_stride, (long)every, anc, u, ess,
                       resampled, log_z);
    return (int)hipGetLastError();
}

extern "C" int cwlt_particle_gather(void* dst, const void* src, const int64_t* anc, int64_t rows, int64_t row_bytes,
                                    int n_blocks, int64_t block_stride, int copy_back, void* stream) {
    using namespace cwlt;
    if (!dst || !src || !anc || dst == src) return CWLT_ERR_ARG;
    if (copy_back < 0 || copy_back > 1 || rows < 1 || rows > (1L << 20) || row_bytes < 4 || row_bytes % 4 ||
        n_blocks < 1 || block_stride % 4 || (n_blocks > 1 && block_stride < rows * row_bytes))
        return CWLT_ERR_ARG;
    const uintptr_t all = (uintptr_t)dst | (uintptr_t)src | (uintptr_t)row_bytes |
                          (n_blocks > 1 ? (uintptr_t)block_stride : 0);
    if (all % 4) return CWLT_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (all % 16 == 0) return launch_gather<uint4>(dst, src, anc, rows, row_bytes, n_blocks, block_stride, copy_back, st);
    if (all % 8 == 0) return launch_gather<uint2>(dst, src, anc, rows, row_bytes, n_blocks, block_stride, copy_back, st);
    return launch_gather<uint32_t>(dst, src, anc, rows, row_bytes, n_blocks, block_stride, copy_back, st);
}
