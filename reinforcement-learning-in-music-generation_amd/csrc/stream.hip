// Continuous batching for generation (generation.generate_stream): a fixed pool of `slots` decode rows on the GEMM step
// (cwlt_decode_step_rows), where a slot whose song has ended starts the next song on the very next token, and the
// device itself decides when a song ends.  Per token the stream enqueues the decode step, then
//   cwlt_stream_refill             copy the song-start snapshot (state + logits) into the slots flagged fresh,
//   cwlt_sample_categorical_keyed  draw each slot's token keyed by (song index, position in song)  (sample.hip),
//   cwlt_stream_advance            record the draw in the output ring, advance position / bar count, detect the song's
//                                  end and hand finished slots the next song indices in slot order.
// All four are fixed launches on fixed buffers, so the whole token is one captured hipGraph.
//
// Per-song prompts (generate_stream(prompts=...)) swap the refill and the advance for their bank forms:
//   cwlt_stream_refill_bank    copy song k's own start (state + logits) from entry k % bank of a device ring of
//                              prefilled songs (the bank) into the slot song k was just handed,
//   cwlt_stream_advance_bank   cwlt_stream_advance with per-song bar0 / cap read from the bank, and a gate: a slot takes
//                              the next song only once the host has marked that song's bank entry written (ctl[3]).
#include "cwlt_common.h"

namespace cwlt {

// One block per CU-sized share of a slot's state: every block walks the fresh flags (a ballot per 64 slots) and, for
// each flagged slot, copies its 1/gridDim share of the snapshot.  The slot layout is DecodeSession._state: per layer
// S of all slots ([slots][s4] float4) then Z of all slots ([slots][z4] float4); the snapshot is the same for one slot.
__global__ __launch_bounds__(256) void stream_refill_kernel(float4* __restrict__ state, const float4* __restrict__ snap,
                                                            long slots, int n_layer, long s4, long z4,
                                                            float* __restrict__ logits,
                                                            const float* __restrict__ snap_logits, long n_logits,
                                                            long ld_logits, const int64_t* __restrict__ fresh) {
    __shared__ unsigned long long mask_s[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long per = s4 + z4, total = (long)n_layer * per;
    const long first = (long)blockIdx.x * blockDim.x + tid, stride = (long)gridDim.x * blockDim.x;
    for (long base = 0; base < slots; base += 256) {
        const long s = base + tid;
        const bool f = s < slots && fresh[s] != 0;
        const unsigned long long m = __ballot(f);
        if (lane == 0) mask_s[w] = m;
        __syncthreads();
        unsigned long long masks[4] = {mask_s[0], mask_s[1], mask_s[2], mask_s[3]};
        __syncthreads();                             // mask_s is rewritten by the next chunk
        for (int q = 0; q < 4; ++q) {
            while (masks[q]) {                       // block-uniform
                const int bit = __builtin_ctzll(masks[q]);
                masks[q] &= masks[q] - 1;
                const long slot = base + q * 64 + bit;
                for (long j = first; j < total; j += stride) {
                    const long layer = j / per, r = j - layer * per;
                    const long d = layer * slots * per + (r < s4 ? slot * s4 + r : slots * s4 + slot * z4 + (r - s4));
                    state[d] = snap[j];
                }
                for (long j = first; j < n_logits; j += stride) logits[slot * ld_logits + j] = snap_logits[j];
            }
        }
    }
}

// One workgroup: slots in chunks of blockDim, the finished slots ranked in slot order by a ballot prefix per wave and
// the wave totals.  ctl = {tokens advanced, songs assigned, songs finished}.
__global__ __launch_bounds__(1024) void stream_advance_kernel(
    const int64_t* __restrict__ tokens, int n_attr, long slots, int bar_attr, const int* __restrict__ bar_mask,
    int bar_classes, long bar_cond, long bar0, long cap, long n_songs, int64_t* __restrict__ song,
    int64_t* __restrict__ pos, int64_t* __restrict__ bar, int64_t* __restrict__ fresh, int64_t* __restrict__ ctl,
    int64_t* __restrict__ ring, long ring_rows) {
    __shared__ int wave_n[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n_wave = blockDim.x >> 6;
    const long t = ctl[0], assigned = ctl[1];
    const long row = t % ring_rows;
    long carry = 0;                                  // finished slots before this chunk
    for (long base = 0; base < slots; base += blockDim.x) {
        const long s = base + tid;
        const bool active = s < slots;
        int ended = 0;
        if (active) {
            const long sg = song[s];
            int64_t* out = ring + (row * slots + s) * (n_attr + 2);
            out[0] = sg;
            for (int a = 0; a < n_attr; ++a) out[1 + a] = tokens[s * n_attr + a];
            if (sg >= 0) {
                const long p = pos[s];
                long b = bar[s];
                const long tk = tokens[s * n_attr + bar_attr];
                if (tk >= 0 && tk < bar_classes && bar_mask[tk]) ++b;
                ended = (b >= bar_cond || p + 1 >= cap) ? 1 : 0;
                pos[s] = p + 1;
                bar[s] = b;
            }
            out[n_attr + 1] = ended;
        }
        const unsigned long long m = __ballot(ended != 0);
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_n[w] = __popcll(m);
        __syncthreads();
        int before = 0, chunk_n = 0;
        for (int q = 0; q < n_wave; ++q) {
            before += q < w ? wave_n[q] : 0;
            chunk_n += wave_n[q];
        }
        __syncthreads();                             // wave_n is rewritten by the next chunk
        if (active) {
            if (ended) {
                const long idx = assigned + carry + before + rank;
                if (idx < n_songs) {
                    song[s] = idx;
                    pos[s] = 0;
                    bar[s] = bar0;
                } else {
                    song[s] = -1;                    // no song left: idle (refilled once, then stepped and ignored)
                }
                fresh[s] = 1;
            } else {
                fresh[s] = 0;
            }
        }
        carry += chunk_n;
    }
    if (tid == 0) {
        ctl[0] = t + 1;
        ctl[1] = assigned + carry < n_songs ? assigned + carry : n_songs;
        ctl[2] = ctl[2] + carry;
    }
}

// stream_refill_kernel's walk, the source of slot s the bank entry song[s] % bank: per layer the S rows of all `bank`
// entries then their Z rows (DecodeSession._state of a `bank`-slot session).  Fresh slots with song < 0 are skipped.
__global__ __launch_bounds__(256) void stream_refill_bank_kernel(float4* __restrict__ state,
                                                                 const float4* __restrict__ bank_state, long bank,
                                                                 long slots, int n_layer, long s4, long z4,
                                                                 float* __restrict__ logits,
                                                                 const float* __restrict__ bank_logits, long n_logits,
                                                                 long ld_logits, long ld_bank_logits,
                                                                 const int64_t* __restrict__ fresh,
                                                                 const int64_t* __restrict__ song) {
    __shared__ unsigned long long mask_s[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long per = s4 + z4, total = (long)n_layer * per;
    const long first = (long)blockIdx.x * blockDim.x + tid, stride = (long)gridDim.x * blockDim.x;
    for (long base = 0; base < slots; base += 256) {
        const long s = base + tid;
        const bool f = s < slots && fresh[s] != 0 && song[s] >= 0;
        const unsigned long long m = __ballot(f);
        if (lane == 0) mask_s[w] = m;
        __syncthreads();
        unsigned long long masks[4] = {mask_s[0], mask_s[1], mask_s[2], mask_s[3]};
        __syncthreads();                             // mask_s is rewritten by the next chunk
        for (int q = 0; q < 4; ++q) {
            while (masks[q]) {                       // block-uniform
                const int bit = __builtin_ctzll(masks[q]);
                masks[q] &= masks[q] - 1;
                const long slot = base + q * 64 + bit;
                const long e = song[slot] % bank;
                for (long j = first; j < total; j += stride) {
                    const long layer = j / per, r = j - layer * per;
                    const long d = layer * slots * per + (r < s4 ? slot * s4 + r : slots * s4 + slot * z4 + (r - s4));
                    const long src = layer * bank * per + (r < s4 ? e * s4 + r : bank * s4 + e * z4 + (r - s4));
                    state[d] = bank_state[src];
                }
                for (long j = first; j < n_logits; j += stride)
                    logits[slot * ld_logits + j] = bank_logits[e * ld_bank_logits + j];
            }
        }
    }
}

// stream_advance_kernel with per-song bar0 / cap and the ready gate.  Candidates for a new song: slots whose song ended
// on this token and slots already waiting (song -2).  They are ranked in slot order; the first min(ready, n_songs) -
// assigned of them take songs (bar0 and cap from the song's bank entry, the cap kept per slot), the rest wait while
// songs remain and go idle (-1) once all are assigned.  Waiting and idle slots write song -1 into the ring row.
// ctl = {tokens advanced, songs assigned, songs finished, songs ready}.
__global__ __launch_bounds__(1024) void stream_advance_bank_kernel(
    const int64_t* __restrict__ tokens, int n_attr, long slots, int bar_attr, const int* __restrict__ bar_mask,
    int bar_classes, long bar_cond, const int64_t* __restrict__ bank_bar0, const int64_t* __restrict__ bank_cap,
    long bank, long n_songs, int64_t* __restrict__ song, int64_t* __restrict__ pos, int64_t* __restrict__ bar,
    int64_t* __restrict__ cap, int64_t* __restrict__ fresh, int64_t* __restrict__ ctl, int64_t* __restrict__ ring,
    long ring_rows) {
    __shared__ int wave_n[16], wave_e[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n_wave = blockDim.x >> 6;
    const long t = ctl[0], assigned = ctl[1], ready = ctl[3];
    const long limit = ready < n_songs ? ready : n_songs;      // song indices below this may be handed out
    const long row = t % ring_rows;
    long carry = 0, carry_e = 0;                     // candidates / ended slots before this chunk
    for (long base = 0; base < slots; base += blockDim.x) {
        const long s = base + tid;
        const bool active = s < slots;
        int ended = 0, cand = 0;
        if (active) {
            const long sg = song[s];
            int64_t* out = ring + (row * slots + s) * (n_attr + 2);
            out[0] = sg >= 0 ? sg : -1;
            for (int a = 0; a < n_attr; ++a) out[1 + a] = tokens[s * n_attr + a];
            if (sg >= 0) {
                const long p = pos[s];
                long b = bar[s];
                const long tk = tokens[s * n_attr + bar_attr];
                if (tk >= 0 && tk < bar_classes && bar_mask[tk]) ++b;
                ended = (b >= bar_cond || p + 1 >= cap[s]) ? 1 : 0;
                pos[s] = p + 1;
                bar[s] = b;
            }
            out[n_attr + 1] = ended;
            cand = (ended || sg == -2) ? 1 : 0;
        }
        const unsigned long long m = __ballot(cand != 0);
        const unsigned long long me = __ballot(ended != 0);
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) {
            wave_n[w] = __popcll(m);
            wave_e[w] = __popcll(me);
        }
        __syncthreads();
        int before = 0, chunk_n = 0, chunk_e = 0;
        for (int q = 0; q < n_wave; ++q) {
            before += q < w ? wave_n[q] : 0;
            chunk_n += wave_n[q];
            chunk_e += wave_e[q];
        }
        __syncthreads();                             // wave_n / wave_e are rewritten by the next chunk
        if (active) {
            int f = 0;
            if (cand) {
                const long idx = assigned + carry + before + rank;
                if (idx < limit) {
                    const long e = idx % bank;
                    song[s] = idx;
                    pos[s] = 0;
                    bar[s] = bank_bar0[e];
                    cap[s] = bank_cap[e];
                    f = 1;
                } else {
                    song[s] = idx < n_songs ? -2 : -1;   // wait for the song's entry, or idle: none left
                }
            }
            fresh[s] = f;
        }
        carry += chunk_n;
        carry_e += chunk_e;
    }
    if (tid == 0) {
        const long room = limit > assigned ? limit - assigned : 0;
        ctl[0] = t + 1;
        ctl[1] = assigned + (carry < room ? carry : room);
        ctl[2] = ctl[2] + carry_e;
    }
}

}  // namespace cwlt

extern "C" int cwlt_stream_refill(float* state, const float* snap_state, int n_layer, int64_t s_floats,
                                  int64_t z_floats, float* logits, const float* snap_logits, int64_t n_logits,
                                  int64_t ld_logits, const int64_t* fresh, int64_t slots, void* stream) {
    using namespace cwlt;
    if (!state || !snap_state || !logits || !snap_logits || !fresh) return CWLT_ERR_ARG;
    if (n_layer < 1 || slots < 1 || s_floats < 4 || z_floats < 4 || s_floats % 4 || z_floats % 4 || n_logits < 1 ||
        ld_logits < n_logits)
        return CWLT_ERR_ARG;
    if (((uintptr_t)state | (uintptr_t)snap_state) % 16) return CWLT_ERR_ARG;
    const long total = (long)n_layer * ((s_floats + z_floats) / 4);
    long blocks = (total + 255) / 256;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(stream_refill_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (float4*)state, (const float4*)snap_state, (long)slots, n_layer, (long)s_floats / 4,
                       (long)z_floats / 4, logits, snap_logits, (long)n_logits, (long)ld_logits, fresh);
    return (int)hipGetLastError();
}

extern "C" int cwlt_stream_advance(const int64_t* tokens, int n_attr, int64_t slots, int bar_attr, const int* bar_mask,
                                   int bar_classes, int64_t bar_cond, int64_t bar0, int64_t cap, int64_t n_songs,
                                   int64_t* song, int64_t* pos, int64_t* bar, int64_t* fresh, int64_t* ctl,
                                   int64_t* ring, int64_t ring_rows, void* stream) {
    using namespace cwlt;
    if (!tokens || !bar_mask || !song || !pos || !bar || !fresh || !ctl || !ring) return CWLT_ERR_ARG;
    if (n_attr < 1 || n_attr > 8 || bar_attr < 0 || bar_attr >= n_attr || bar_classes < 1 || slots < 1 ||
        ring_rows < 1 || cap < 1 || n_songs < 0 || n_songs > (1L << 20) || bar0 >= bar_cond)
        return CWLT_ERR_ARG;
    hipLaunchKernelGGL(stream_advance_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, tokens, n_attr, (long)slots,
                       bar_attr, bar_mask, bar_classes, (long)bar_cond, (long)bar0, (long)cap, (long)n_songs, song, pos,
                       bar, fresh, ctl, ring, (long)ring_rows);
    return (int)hipGetLastError();
}

extern "C" int cwlt_stream_refill_bank(float* state, const float* bank_state, int64_t bank, int n_layer,
                                       int64_t s_floats, int64_t z_floats, float* logits, const float* bank_logits,
                                       int64_t n_logits, int64_t ld_logits, int64_t ld_bank_logits,
                                       const int64_t* fresh, const int64_t* song, int64_t slots, void* stream) {
    using namespace cwlt;
    if (!state || !bank_state || !logits || !bank_logits || !fresh || !song) return CWLT_ERR_ARG;
    if (n_layer < 1 || slots < 1 || bank < 1 || s_floats < 4 || z_floats < 4 || s_floats % 4 || z_floats % 4 ||
        n_logits < 1 || ld_logits < n_logits || ld_bank_logits < n_logits)
        return CWLT_ERR_ARG;
    if (((uintptr_t)state | (uintptr_t)bank_state) % 16) return CWLT_ERR_ARG;
    const long total = (long)n_layer * ((s_floats + z_floats) / 4);
    long blocks = (total + 255) / 256;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(stream_refill_bank_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (float4*)state, (const float4*)bank_state, (long)bank, (long)slots, n_layer,
                       (long)s_floats / 4, (long)z_floats / 4, logits, bank_logits, (long)n_logits, (long)ld_logits,
                       (long)ld_bank_logits, fresh, song);
    return (int)hipGetLastError();
}

extern "C" int cwlt_stream_advance_bank(const int64_t* tokens, int n_attr, int64_t slots, int bar_attr,
                                        const int* bar_mask, int bar_classes, int64_t bar_cond,
                                        const int64_t* bank_bar0, const int64_t* bank_cap, int64_t bank,
                                        int64_t n_songs, int64_t* song, int64_t* pos, int64_t* bar, int64_t* cap,
                                        int64_t* fresh, int64_t* ctl, int64_t* ring, int64_t ring_rows,
                                        void* stream) {
    using namespace cwlt;
    if (!tokens || !bar_mask || !bank_bar0 || !bank_cap || !song || !pos || !bar || !cap || !fresh || !ctl || !ring)
        return CWLT_ERR_ARG;
    if (n_attr < 1 || n_attr > 8 || bar_attr < 0 || bar_attr >= n_attr || bar_classes < 1 || slots < 1 ||
        ring_rows < 1 || bank < 1 || n_songs < 0 || n_songs > (1L << 20) || bar_cond < 1)
        return CWLT_ERR_ARG;
    hipLaunchKernelGGL(stream_advance_bank_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, tokens, n_attr,
                       (long)slots, bar_attr, bar_mask, bar_classes, (long)bar_cond, bank_bar0, bank_cap, (long)bank,
                       (long)n_songs, song, pos, bar, cap, fresh, ctl, ring, (long)ring_rows);
    return (int)hipGetLastError();
}
