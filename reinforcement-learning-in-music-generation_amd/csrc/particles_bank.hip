// Per-song prompts on the particle stream (generation.generate_particles(slots=, prompts=[...], bank=)):
// every song starts from its own entry, song % bank, of the device bank of prefilled prompts that generate_stream's
// per-song form keeps (stream.hip), and the K particles of a song share that one prefill.
//   cwlt_particle_refill_bank   per token, inside the captured token, in the place of cwlt_stream_refill: the fresh rows
//                               of a group take the state and logits of their song's entry -- each float4 of the entry
//                               loaded once and stored to every fresh row of the group.
// The hand-out of songs at a boundary, cwlt_particle_release_bank, is particle_release_kernel<true> in
// particles_stream.hip.
// One launch, no host synchronisation, no allocation, no atomics, no cross-workgroup communication; every barrier
// is workgroup-uniform; all index arithmetic is 64-bit.
#include "cwlt_common.h"

namespace cwlt {

constexpr int GROUP_WORDS = 16;                      // 64-row words of one group's flags: K <= 1024

// Every block walks the rows' flags, a ballot per 64 rows (stream_refill_kernel's scan); nothing fresh: nothing else.
// The first flagged row of a group makes the block serve the whole group: its K flags are read again, 256 at a time,
// into `todo_s`; the rows among them that take the leader's entry (all of them, after a release) form `same_s`, and
// the block's 1/gridDim share of that entry goes to each of them, one load per float4.  Rows of the group that asked
// for another entry stay in `todo_s` for another pass, so a row's source is always (id[n] / K) % bank.
__global__ __launch_bounds__(256) void particle_refill_bank_kernel(
    float4* __restrict__ state, const float4* __restrict__ src, long bank, long rows, int K, int n_layer, long s4,
    long z4, float* __restrict__ logits, const float* __restrict__ src_logits, long n_logits, long ld_logits,
    long ld_src_logits, const int64_t* __restrict__ fresh, const int64_t* __restrict__ id) {
    __shared__ unsigned long long mask_s[4];
    __shared__ unsigned long long todo_s[GROUP_WORDS], same_s[GROUP_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long per = s4 + z4, total = (long)n_layer * per;
    const long first = (long)blockIdx.x * blockDim.x + tid, stride = (long)gridDim.x * blockDim.x;
    const int words = (K + 63) >> 6;
    long served = -1;                                // the last group served: the scan meets its later rows again
    for (long base = 0; base < rows; base += 256) {
        const long n = base + tid;
        const bool f = n < rows && fresh[n] != 0 && id[n] >= 0;
        const unsigned long long m = __ballot(f);
        if (lane == 0) mask_s[w] = m;
        __syncthreads();
        unsigned long long masks[4] = {mask_s[0], mask_s[1], mask_s[2], mask_s[3]};
        __syncthreads();                             // mask_s is rewritten by the next chunk
        for (int q = 0; q < 4; ++q) {
            while (masks[q]) {                       // block-uniform
                const int bit = __builtin_ctzll(masks[q]);
                masks[q] &= masks[q] - 1;
                const long g = (base + q * 64 + bit) / K;
                if (g <= served) continue;
                served = g;
                const long row0 = g * K;
                long ent[4];                         // this thread's rows row0 + tid + 256 i: their entries, -1: none
                for (int i = 0; i < 4; ++i) {
                    const long k = tid + 256L * i;
                    ent[i] = -1;
                    if (k < K && fresh[row0 + k] != 0 && id[row0 + k] >= 0) ent[i] = (id[row0 + k] / K) % bank;
                }
                for (int i = 0; i < 4; ++i) {
                    const unsigned long long t = __ballot(ent[i] >= 0);
                    if (lane == 0 && i * 4 + w < words) todo_s[i * 4 + w] = t;
                }
                __syncthreads();
                for (;;) {                           // block-uniform: one pass per distinct entry, one after a release
                    long lead = -1;
                    for (int x = 0; x < words && lead < 0; ++x)
                        if (todo_s[x]) lead = x * 64 + __builtin_ctzll(todo_s[x]);
                    __syncthreads();                 // every thread has read todo_s: it is rewritten below, or by the
                    if (lead < 0) break;             // next group
                    const long e = (id[row0 + lead] / K) % bank;
                    for (int i = 0; i < 4; ++i) {
                        const bool hit = ent[i] == e;
                        const unsigned long long t = __ballot(hit);
                        if (lane == 0 && i * 4 + w < words) {
                            same_s[i * 4 + w] = t;
                            todo_s[i * 4 + w] &= ~t;
                        }
                        if (hit) ent[i] = -1;
                    }
                    __syncthreads();
                    for (long j = first; j < total; j += stride) {
                        const long layer = j / per, r = j - layer * per;
                        const float4 v = src[layer * bank * per + (r < s4 ? e * s4 + r : bank * s4 + e * z4 + (r - s4))];
                        const long d0 = layer * rows * per;
                        for (int x = 0; x < words; ++x) {
                            unsigned long long t = same_s[x];
                            while (t) {
                                const long row = row0 + x * 64 + __builtin_ctzll(t);
                                t &= t - 1;
                                state[d0 + (r < s4 ? row * s4 + r : rows * s4 + row * z4 + (r - s4))] = v;
                            }
                        }
                    }
                    const float* from = src_logits + e * ld_src_logits;
                    for (long j = first; j < n_logits; j += stride) {
                        const float v = from[j];
                        for (int x = 0; x < words; ++x) {
                            unsigned long long t = same_s[x];
                            while (t) {
                                const long row = row0 + x * 64 + __builtin_ctzll(t);
                                t &= t - 1;
                                logits[row * ld_logits + j] = v;
                            }
                        }
                    }
                    __syncthreads();                 // same_s is rewritten by the next pass or group
                }
            }
        }
    }
}

}  // namespace cwlt

extern "C" int cwlt_particle_refill_bank(float* state, const float* bank_state, int64_t bank, int n_layer,
                                         int64_t s_floats, int64_t z_floats, float* logits, const float* bank_logits,
                                         int64_t n_logits, int64_t ld_logits, int64_t ld_bank_logits,
                                         const int64_t* fresh, const int64_t* id, int64_t rows, int particles,
                                         void* stream) {
    using namespace cwlt;
    if (!state || !bank_state || !logits || !bank_logits || !fresh || !id) return CWLT_ERR_ARG;
    if (n_layer < 1 || bank < 1 || rows < 1 || rows > (1L << 20) || particles < 2 || particles > 1024 ||
        rows % particles || s_floats < 4 || z_floats < 4 || s_floats % 4 || z_floats % 4 || n_logits < 1 ||
        ld_logits < n_logits || ld_bank_logits < n_logits)
        return CWLT_ERR_ARG;
    if (((uintptr_t)state | (uintptr_t)bank_state) % 16) return CWLT_ERR_ARG;
    const long total = (long)n_layer * ((s_floats + z_floats) / 4);
    long blocks = (total + 255) / 256;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(particle_refill_bank_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (float4*)state, (const float4*)bank_state, (long)bank, (long)rows, particles, n_layer,
                       (long)s_floats / 4, (long)z_floats / 4, logits, bank_logits, (long)n_logits, (long)ld_logits,
                       (long)ld_bank_logits, fresh, id);
    return (int)hipGetLastError();
}
