// Per-song prompts on the particle stream (generation.generate_particles(slots=, prompts=[...], bank=)):
// every song starts from its own entry, song % bank, of the device bank of prefilled prompts that generate_stream's
// per-song form keeps (stream.hip), and the K particles of a song share that one prefill.
//   cwlt_particle_refill_bank   per token, inside the captured token, in the place of cwlt_stream_refill: the fresh rows
//                               of a group take the state and logits of their song's entry -- each float4 of the entry
//                               loaded once and stored to every fresh row of the group;
//   cwlt_particle_release_bank  per hand-out boundary, in the place of cwlt_particle_release: the same ranking of the
//                               groups that can take a song, but songs are handed out only below min(ctl[3], n_songs),
//                               ctl[3] the songs whose entries the host has marked written, and a row handed song v starts
//                               from bar0_all[v] and cap_all[v], two tables of n_songs entries, not from two scalars.
// One launch each, no host synchronisation, no allocation, no atomics, no cross-workgroup communication; every barrier
// is workgroup-uniform; all index arithmetic is 64-bit.
#include "cwlt_common.h"

namespace cwlt {

constexpr int BANK_RELEASE_GROUPS = 4096;            // groups of one release: its decisions live in LDS
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

// particle_release_kernel (particles_stream.hip) with the gate and the tables, and nothing else changed: one workgroup;
// phase 1, one thread per group, ranks the candidates -- no song, or every row done -- in group order, and candidate
// number r takes song ctl[1] + r while that lies below limit = min(ctl[3], n_songs), else none (-1: parked, a candidate
// again at the next boundary); a candidate that had a song is finished and its outputs are written whether or not the
// group gets a new one.  Phase 2, one thread per row: a handed row starts from bar0_all / cap_all of its new song.
__global__ __launch_bounds__(1024) void particle_release_bank_kernel(
    long groups, int K, long n_songs, const int64_t* __restrict__ bar0_all, const int64_t* __restrict__ cap_all,
    int64_t* __restrict__ song, int64_t* __restrict__ id, int64_t* __restrict__ pos, int64_t* __restrict__ bar,
    int64_t* __restrict__ cap, int64_t* __restrict__ len, int64_t* __restrict__ done, int64_t* __restrict__ fresh,
    float* __restrict__ lw, float* __restrict__ log_z, int64_t* __restrict__ ctl, float* __restrict__ out_lw,
    int64_t* __restrict__ out_len, float* __restrict__ out_logz) {
    __shared__ int take_s[BANK_RELEASE_GROUPS];      // -2: no candidate; -1: parked; else the song handed out
    __shared__ int wave_n[16], wave_f[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n_wave = blockDim.x >> 6;
    const long assigned = ctl[1], ready = ctl[3];
    const long limit = ready < n_songs ? ready : n_songs;
    long carry = 0, carry_f = 0;                     // candidates / finished songs before this chunk
    for (long base = 0; base < groups; base += blockDim.x) {
        const long g = base + tid;
        const bool active = g < groups;
        int cand = 0, fin = 0;
        long sg = -1;
        if (active) {
            sg = song[g];
            int all = 1;
            for (int k = 0; k < K; ++k) all &= done[g * K + k] != 0 ? 1 : 0;
            cand = (sg < 0 || all) ? 1 : 0;
            fin = (sg >= 0 && all) ? 1 : 0;
        }
        const unsigned long long m = __ballot(cand != 0);
        const unsigned long long mf = __ballot(fin != 0);
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) {
            wave_n[w] = __popcll(m);
            wave_f[w] = __popcll(mf);
        }
        __syncthreads();
        int before = 0, chunk_n = 0, chunk_f = 0;
        for (int q = 0; q < n_wave; ++q) {
            before += q < w ? wave_n[q] : 0;
            chunk_n += wave_n[q];
            chunk_f += wave_f[q];
        }
        __syncthreads();                             // wave_n / wave_f are rewritten by the next chunk
        if (active) {
            int v = -2;
            if (cand) {
                const long idx = assigned + carry + before + rank;
                v = idx < limit ? (int)idx : -1;
                if (fin && sg < n_songs) out_logz[sg] = log_z[g];
                song[g] = v;
                if (v >= 0) log_z[g] = 0.f;
            }
            take_s[g] = v;
        }
        carry += chunk_n;
        carry_f += chunk_f;
    }
    __syncthreads();
    const long rows = groups * K;
    for (long n = tid; n < rows; n += blockDim.x) {
        const long g = n / K;
        const int v = take_s[g];
        if (v == -2) continue;
        const long old = id[n];
        if (old >= 0 && old < n_songs * K) {       // the output arrays hold n_songs * K particles
            out_lw[old] = lw[n];
            out_len[old] = len[n];
        }
        if (v >= 0) {                                // v < limit <= n_songs: inside the tables
            id[n] = (long)v * K + (n - g * K);
            pos[n] = 0;
            bar[n] = bar0_all[v];
            cap[n] = cap_all[v];
            len[n] = 0;
            done[n] = 0;
            lw[n] = 0.f;
            fresh[n] = 1;
        } else {
            id[n] = -1;
            done[n] = 1;
        }
    }
    if (tid == 0) {
        const long next = assigned + carry, top = limit > assigned ? limit : assigned;
        ctl[1] = next > top ? top : next;            // never decreases
        ctl[2] = ctl[2] + carry_f;
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

extern "C" int cwlt_particle_release_bank(int64_t groups, int particles, int64_t n_songs, const int64_t* bar0_all,
                                          const int64_t* cap_all, int64_t* song, int64_t* id, int64_t* pos,
                                          int64_t* bar, int64_t* cap, int64_t* len, int64_t* done, int64_t* fresh,
                                          float* lw, float* log_z, int64_t* ctl, float* out_lw, int64_t* out_len,
                                          float* out_logz, void* stream) {
    using namespace cwlt;
    if (!bar0_all || !cap_all || !song || !id || !pos || !bar || !cap || !len || !done || !fresh || !lw || !log_z ||
        !ctl || !out_lw || !out_len || !out_logz)
        return CWLT_ERR_ARG;
    if (particles < 2 || particles > 1024 || groups < 1 || groups > BANK_RELEASE_GROUPS ||
        groups * particles > (1L << 20) || n_songs < 0 || n_songs * particles > (1L << 20))
        return CWLT_ERR_ARG;
    hipLaunchKernelGGL(particle_release_bank_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (long)groups,
                       particles, (long)n_songs, bar0_all, cap_all, song, id, pos, bar, cap, len, done, fresh, lw, log_z,
                       ctl, out_lw, out_len, out_logz);
    return (int)hipGetLastError();
}
