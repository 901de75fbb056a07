// Particle generation on the stream (generation.generate_particles(slots=)): a pool of S groups of K
// consecutive decode rows in which a group whose K particles have all ended takes the next song, at the next resampling
// boundary.  Beside the kernels of particles.hip (cwlt_particle_weigh per token; cwlt_particle_resample_keyed and
// cwlt_particle_gather per event) and cwlt_stream_refill:
//   cwlt_particle_advance  per token, inside the captured token, after cwlt_particle_weigh: (particle id, token, done)
//                          into the output ring's row ctl[0] % ring_rows, the rows' clocks ticked, every fresh flag
//                          cleared, ctl[0] moved;
//   cwlt_particle_release  per event, after the gather: one workgroup ranks the groups that can take a song -- every row
//                          done, or no song -- in group order, writes a finished song's final weights, lengths and
//                          evidence into the run's output arrays and hands out the next song indices;
//   cwlt_particle_release_bank  the same kernel's other instantiation, for per-song prompts (particles_bank.hip, DESIGN
//                          §4.6q): songs are handed out only below min(ctl[3], n_songs), and a row handed song v starts
//                          from bar0_all[v] and cap_all[v], two tables of n_songs entries, not from two scalars;
//   cwlt_particle_fill     per event, after the release: dst[n] = src[id[n]] for the rows flagged fresh -- the new
//                          particles' grammar positions and repetition states.
// One launch each, no host synchronisation, no allocation, no atomics, no cross-workgroup communication; every barrier
// is workgroup-uniform; all index arithmetic is 64-bit.
#include "cwlt_common.h"

namespace cwlt {

constexpr int RELEASE_GROUPS = 4096;                 // groups of one release: its decisions live in LDS

// One workgroup, rows in chunks of blockDim.  Every thread reads ctl[0] ahead of the barrier; thread 0 moves it last.
__global__ __launch_bounds__(1024) void particle_advance_kernel(const int64_t* __restrict__ tokens, int n_attr,
                                                                long rows, const int64_t* __restrict__ id,
                                                                const int64_t* __restrict__ done,
                                                                int64_t* __restrict__ pos, int64_t* __restrict__ fresh,
                                                                int64_t* __restrict__ ctl, int64_t* __restrict__ ring,
                                                                long ring_rows) {
    const long t = ctl[0];
    __syncthreads();
    const long row = t % ring_rows;
    for (long n = threadIdx.x; n < rows; n += blockDim.x) {
        const long i = id[n];
        int64_t* out = ring + (row * rows + n) * (n_attr + 2);
        out[0] = i >= 0 ? i : -1;
        for (int a = 0; a < n_attr; ++a) out[1 + a] = tokens[n * n_attr + a];
        out[n_attr + 1] = (i >= 0 && done[n] != 0) ? 1 : 0;
        if (i >= 0) pos[n] = pos[n] + 1;
        fresh[n] = 0;
    }
    if (threadIdx.x == 0) ctl[0] = t + 1;
}

// Where a handed-out row's bar count and cap come from: two scalars, or (BANK) two tables of n_songs entries.
template <bool BANK>
struct ParticleStart {
    long bar0, cap;
};
template <>
struct ParticleStart<true> {
    const int64_t* bar0;                             // [n_songs]
    const int64_t* cap;                              // [n_songs]
};

// A row takes song v -> the bar count and the cap it starts from.
__device__ inline long bar_of(const ParticleStart<false>& st, long) { return st.bar0; }
__device__ inline long bar_of(const ParticleStart<true>& st, long v) { return st.bar0[v]; }
__device__ inline long cap_of(const ParticleStart<false>& st, long) { return st.cap; }
__device__ inline long cap_of(const ParticleStart<true>& st, long v) { return st.cap[v]; }

// One workgroup.  Phase 1, one thread per group, groups in chunks of blockDim: a group is a candidate for a song when it
// has none or when its K rows are all done; candidates are ranked in group order by a ballot prefix per wave, the wave
// totals and the chunks before (stream_advance_kernel's ranking), and candidate number r takes song ctl[1] + r while
// that lies below limit, else none (-1: parked, a candidate again at the next boundary).  limit is n_songs, lowered
// (BANK) to ctl[3], the songs whose bank entries the host has marked written; the plain form's ctl has no ctl[3].  A
// candidate that had a song is finished: its log_z goes to out_logz[song], whether or not the group gets a new one.
// Phase 2, after the barrier, one thread per row: a candidate group's rows write their particle's final lw and len to
// out_lw / out_len[id] (when they had one) and are then set up for the new song, or parked (id -1, done 1).  The rows of
// a group that is no candidate, and its song and log_z, are not written.
template <bool BANK>
__global__ __launch_bounds__(1024) void particle_release_kernel(
    long groups, int K, long n_songs, ParticleStart<BANK> st, int64_t* __restrict__ song, int64_t* __restrict__ id,
    int64_t* __restrict__ pos, int64_t* __restrict__ bar, int64_t* __restrict__ cap, int64_t* __restrict__ len,
    int64_t* __restrict__ done, int64_t* __restrict__ fresh, float* __restrict__ lw, float* __restrict__ log_z,
    int64_t* __restrict__ ctl, float* __restrict__ out_lw, int64_t* __restrict__ out_len,
    float* __restrict__ out_logz) {
    __shared__ int take_s[RELEASE_GROUPS];           // -2: no candidate; -1: parked; else the song handed out
    __shared__ int wave_n[16], wave_f[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n_wave = blockDim.x >> 6;
    const long assigned = ctl[1];
    long limit = n_songs;                            // song indices below this may be handed out
    if (BANK && ctl[3] < limit) limit = ctl[3];
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
            bar[n] = bar_of(st, v);
            cap[n] = cap_of(st, v);
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
        const long next = assigned + carry;
        const long top = BANK && assigned > limit ? assigned : limit;   // BANK: the counter never decreases
        ctl[1] = next > top ? top : next;
        ctl[2] = ctl[2] + carry_f;
    }
}

// Work items are (row, 4-byte unit); the workgroups grid-stride over them.
__global__ __launch_bounds__(256) void particle_fill_kernel(uint32_t* __restrict__ dst,
                                                            const uint32_t* __restrict__ src,
                                                            const int64_t* __restrict__ fresh,
                                                            const int64_t* __restrict__ id, long rows, long n_src,
                                                            long units, long ld_dst, long ld_src) {
    const long items = rows * units, stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += stride) {
        const long n = i / units, c = i - n * units;
        if (fresh[n] == 0) continue;
        const long k = id[n];
        if (k < 0 || k >= n_src) continue;
        dst[n * ld_dst + c] = src[k * ld_src + c];
    }
}

// The checks and the launch the two release entries share.
template <bool BANK>
static int particle_release(int64_t groups, int particles, int64_t n_songs, ParticleStart<BANK> st, int64_t* song,
                            int64_t* id, int64_t* pos, int64_t* bar, int64_t* cap, int64_t* len, int64_t* done,
                            int64_t* fresh, float* lw, float* log_z, int64_t* ctl, float* out_lw, int64_t* out_len,
                            float* out_logz, void* stream) {
    if (!song || !id || !pos || !bar || !cap || !len || !done || !fresh || !lw || !log_z || !ctl || !out_lw ||
        !out_len || !out_logz)
        return CWLT_ERR_ARG;
    if (particles < 2 || particles > 1024 || groups < 1 || groups > RELEASE_GROUPS ||
        groups * particles > (1L << 20) || n_songs < 0 || n_songs * particles > (1L << 20))
        return CWLT_ERR_ARG;
    hipLaunchKernelGGL(particle_release_kernel<BANK>, dim3(1), dim3(1024), 0, (hipStream_t)stream, (long)groups,
                       particles, (long)n_songs, st, song, id, pos, bar, cap, len, done, fresh, lw, log_z, ctl, out_lw,
                       out_len, out_logz);
    return (int)hipGetLastError();
}

}  // namespace cwlt

extern "C" int cwlt_particle_advance(const int64_t* tokens, int n_attr, int64_t rows, const int64_t* id,
                                     const int64_t* done, int64_t* pos, int64_t* fresh, int64_t* ctl, int64_t* ring,
                                     int64_t ring_rows, void* stream) {
    using namespace cwlt;
    if (!tokens || !id || !done || !pos || !fresh || !ctl || !ring) return CWLT_ERR_ARG;
    if (n_attr < 1 || n_attr > 8 || rows < 1 || rows > (1L << 20) || ring_rows < 1) return CWLT_ERR_ARG;
    hipLaunchKernelGGL(particle_advance_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, tokens, n_attr, (long)rows,
                       id, done, pos, fresh, ctl, ring, (long)ring_rows);
    return (int)hipGetLastError();
}

extern "C" int cwlt_particle_release(int64_t groups, int particles, int64_t n_songs, int64_t bar0, int64_t cap0,
                                     int64_t* song, int64_t* id, int64_t* pos, int64_t* bar, int64_t* cap,
                                     int64_t* len, int64_t* done, int64_t* fresh, float* lw, float* log_z,
                                     int64_t* ctl, float* out_lw, int64_t* out_len, float* out_logz, void* stream) {
    if (cap0 < 1) return CWLT_ERR_ARG;
    return cwlt::particle_release<false>(groups, particles, n_songs, {(long)bar0, (long)cap0}, song, id, pos, bar, cap,
                                         len, done, fresh, lw, log_z, ctl, out_lw, out_len, out_logz, stream);
}

extern "C" int cwlt_particle_release_bank(int64_t groups, int particles, int64_t n_songs, const int64_t* bar0_all,
                                          const int64_t* cap_all, int64_t* song, int64_t* id, int64_t* pos,
                                          int64_t* bar, int64_t* cap, int64_t* len, int64_t* done, int64_t* fresh,
                                          float* lw, float* log_z, int64_t* ctl, float* out_lw, int64_t* out_len,
                                          float* out_logz, void* stream) {
    if (!bar0_all || !cap_all) return CWLT_ERR_ARG;
    return cwlt::particle_release<true>(groups, particles, n_songs, {bar0_all, cap_all}, song, id, pos, bar, cap, len,
                                        done, fresh, lw, log_z, ctl, out_lw, out_len, out_logz, stream);
}

extern "C" int cwlt_particle_fill(void* dst, const void* src, const int64_t* fresh, const int64_t* id, int64_t rows,
                                  int64_t n_src, int64_t row_bytes, int64_t ld_dst, int64_t ld_src, void* stream) {
    using namespace cwlt;
    if (!dst || !src || !fresh || !id || dst == src) return CWLT_ERR_ARG;
    if (rows < 1 || rows > (1L << 20) || n_src < 1 || n_src > (1L << 20) || row_bytes < 4 || row_bytes % 4 ||
        ld_dst < row_bytes || ld_src < row_bytes || ld_dst % 4 || ld_src % 4 ||
        ((uintptr_t)dst | (uintptr_t)src) % 4)
        return CWLT_ERR_ARG;
    const long units = row_bytes / 4;
    long blocks = (rows * units + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(particle_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (uint32_t*)dst,
                       (const uint32_t*)src, fresh, id, (long)rows, (long)n_src, units, (long)ld_dst / 4,
                       (long)ld_src / 4);
    return (int)hipGetLastError();
}
