// Reward-guided particle generation (generation.generate_particles(reward=)): the window of each
// particle's recent rows, kept per pool row so that cwlt_particle_gather hands it from ancestor to descendant, and the
// reward term of the log-weights.  Per token
//   cwlt_reward_push    writes the drawn row, and whether the particle was still alive when it was drawn, into slot
//                       counter % W of the row's ring;
// per reward event (the ring wrapped, or the run ended inside a window)
//   cwlt_reward_window  the ring as the reward callable sees it: tokens and a 0/1 mask of the live slots, zero elsewhere,
//                       and per row whether it has a live slot at all;
//   cwlt_reward_apply   lw += beta * r for the rows that have one, and the reward into the event's history row;
//   cwlt_reward_apply_keyed  the same with the reward weight of the row's own song: beta[s], s the row's
//                       particle id / K -- the row index in the lock-step pool, the stream's id array otherwise.
// None of the four synchronises with the host or allocates: push sits inside the captured token; the window kernel and
// one of the two apply kernels are enqueued between replays, around the callable.  No cross-workgroup communication, no atomics, no barriers.
#include "cwlt_common.h"

namespace cwlt {

// One thread per (row, attribute); the thread of attribute 0 also writes the flag.  `done` is read as the previous
// token's cwlt_particle_weigh left it: the row that ends a song is live.
__global__ __launch_bounds__(256) void reward_push_kernel(const int64_t* __restrict__ tok,
                                                          const int64_t* __restrict__ done,
                                                          const int64_t* __restrict__ counter, long rows, int n_attr,
                                                          long W, int64_t* __restrict__ recent,
                                                          int64_t* __restrict__ live) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * n_attr) return;
    const long n = i / n_attr, a = i - n * n_attr;
    long s = (long)(*counter % W);
    if (s < 0) s += W;                               // a counter never is negative; the slot stays inside the ring
    recent[(n * W + s) * n_attr + a] = tok[i];
    if (a == 0) live[n * W + s] = done[n] == 0 ? 1 : 0;
}

// One thread per (row, slot).  Slot 0's thread also looks through the row's flags: it writes any[n] and stands in for
// the mask of a row without a live slot.
__global__ __launch_bounds__(256) void reward_window_kernel(const int64_t* __restrict__ recent,
                                                            const int64_t* __restrict__ live, long rows, int n_attr,
                                                            long W, long filled, int64_t* __restrict__ win,
                                                            int64_t* __restrict__ mask, int64_t* __restrict__ any) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * W) return;
    const long n = i / W, j = i - n * W;
    const bool on = j < filled && live[i] != 0;
    const int64_t* s = recent + i * n_attr;
    int64_t* d = win + i * n_attr;
    for (int a = 0; a < n_attr; ++a) d[a] = on ? s[a] : 0;
    if (j != 0) {
        mask[i] = on ? 1 : 0;
        return;
    }
    bool some = false;
    for (long q = 0; q < filled; ++q) some = some || live[n * W + q] != 0;
    any[n] = some ? 1 : 0;
    mask[i] = on || !some ? 1 : 0;
}

// The product, then the sum, each rounded on its own (fp contract off: v_mul_f32 + v_add_f32, never an fma).
__device__ inline float reward_term(float lw, float beta, float r) {
#pragma clang fp contract(off)
    const float m = beta * r;
    return lw + m;
}

// One thread per row.  A row without a live slot is skipped by a select: its r may be anything.  Bitwise
// sampling.reward_apply_f32.
__global__ __launch_bounds__(256) void reward_apply_kernel(const float* __restrict__ r,
                                                           const int64_t* __restrict__ any, float beta, long rows,
                                                           float* __restrict__ lw, float* __restrict__ h_r) {
    const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= rows) return;
    const bool on = any[n] != 0;
    const float x = r[n];
    h_r[n] = on ? x : 0.f;
    if (on) lw[n] = reward_term(lw[n], beta, x);
}

// One thread per row, cwlt_reward_apply's arithmetic (reward_term) with beta[s] of the row's song s = id / K, id the
// row's key (NULL: the row index).  A row is on when it has a live slot, an id and a table entry; beta is read for on
// rows only, and an off row is skipped by a select: its r may be anything.  Bitwise sampling.reward_apply_keyed_f32.
__global__ __launch_bounds__(256) void reward_apply_keyed_kernel(const float* __restrict__ r,
                                                                 const int64_t* __restrict__ any,
                                                                 const float* __restrict__ beta, long n_beta,
                                                                 const int64_t* __restrict__ key, long K, long rows,
                                                                 float* __restrict__ lw, float* __restrict__ h_r) {
    const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= rows) return;
    const long id = key ? (long)key[n] : n;
    const long s = id >= 0 ? id / K : -1;
    const bool on = any[n] != 0 && id >= 0 && s < n_beta;
    const float x = r[n];
    h_r[n] = on ? x : 0.f;
    if (on) lw[n] = reward_term(lw[n], beta[s], x);
}

constexpr long REWARD_MAX_ROWS = 1L << 20, REWARD_MAX_WINDOW = 1L << 16;

}  // namespace cwlt

extern "C" int cwlt_reward_push(const int64_t* tok, const int64_t* done, const int64_t* counter, int64_t rows,
                                int n_attr, int64_t window, int64_t* recent, int64_t* live, void* stream) {
    using namespace cwlt;
    if (!tok || !done || !counter || !recent || !live) return CWLT_ERR_ARG;
    if (rows < 1 || rows > REWARD_MAX_ROWS || n_attr < 1 || n_attr > 8 || window < 1 || window > REWARD_MAX_WINDOW)
        return CWLT_ERR_ARG;
    const long threads = (long)rows * n_attr;
    hipLaunchKernelGGL(reward_push_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       tok, done, counter, (long)rows, n_attr, (long)window, recent, live);
    return (int)hipGetLastError();
}

extern "C" int cwlt_reward_window(const int64_t* recent, const int64_t* live, int64_t rows, int n_attr, int64_t window,
                                  int64_t filled, int64_t* win, int64_t* mask, int64_t* any, void* stream) {
    using namespace cwlt;
    if (!recent || !live || !win || !mask || !any) return CWLT_ERR_ARG;
    if (rows < 1 || rows > REWARD_MAX_ROWS || n_attr < 1 || n_attr > 8 || window < 1 || window > REWARD_MAX_WINDOW ||
        filled < 1 || filled > window)
        return CWLT_ERR_ARG;
    const long threads = (long)rows * window;
    hipLaunchKernelGGL(reward_window_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       recent, live, (long)rows, n_attr, (long)window, (long)filled, win, mask, any);
    return (int)hipGetLastError();
}

extern "C" int cwlt_reward_apply(const float* r, const int64_t* any, float beta, int64_t rows, float* lw, float* h_r,
                                 void* stream) {
    using namespace cwlt;
    if (!r || !any || !lw || !h_r) return CWLT_ERR_ARG;
    if (rows < 1 || rows > REWARD_MAX_ROWS) return CWLT_ERR_ARG;
    hipLaunchKernelGGL(reward_apply_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, r,
                       any, beta, (long)rows, lw, h_r);
    return (int)hipGetLastError();
}

extern "C" int cwlt_reward_apply_keyed(const float* r, const int64_t* any, const float* beta, int64_t n_beta,
                                       const int64_t* key, int particles, int64_t rows, float* lw, float* h_r,
                                       void* stream) {
    using namespace cwlt;
    if (!r || !any || !beta || !lw || !h_r) return CWLT_ERR_ARG;
    if (rows < 1 || rows > REWARD_MAX_ROWS || n_beta < 1 || particles < 1) return CWLT_ERR_ARG;
    hipLaunchKernelGGL(reward_apply_keyed_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, r, any, beta, (long)n_beta, key, (long)particles, (long)rows, lw, h_r);
    return (int)hipGetLastError();
}
