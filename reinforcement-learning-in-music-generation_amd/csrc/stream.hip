// Continuous batching for generation (generation.generate_stream): a fixed pool of `slots` decode rows on the GEMM step
// (cwlt_decode_step_rows), where a slot whose song has ended starts the next song on the very next token, and the
// device itself decides when a song ends.  Per token the stream enqueues the decode step, then
//   cwlt_stream_refill             copy the song-start snapshot (state + logits) into the slots flagged fresh,
//   cwlt_sample_categorical_keyed  draw each slot's token keyed by (song index, position in song)  (sample.hip),
//   cwlt_stream_advance            record the draw in the output ring, advance position / bar count, detect the song's
//                                  end and hand finished slots the next song indices in slot order.
// All four are fixed launches on fixed buffers, so the whole token is one captured hipGraph.
//
// Per-song prompts (generate_stream(prompts=...)) run cwlt_stream_refill_bank and cwlt_stream_advance_bank instead: the
// same two kernels instantiated with BANK.  Every song then starts from its own entry, k % bank, of a device ring of
// prefilled songs (the bank), and that is all BANK changes:
//   refill    the source of a fresh slot is its song's entry, not the one snapshot, and a fresh slot with song < 0 has
//             no entry and is skipped (the plain form copies the snapshot into a slot going idle as well);
//   advance   bar0 and cap are read from the new song's entry (the cap kept per slot: the entry is reused later), not
//             passed as two scalars; and songs are handed out only below min(ctl[3], n_songs), ctl[3] the songs whose
//             entries the host has marked written, not below n_songs.  A candidate past that limit waits (song -2) while
//             songs remain and is a candidate again on the next token; it is flagged fresh only once it has a song.
//             Waiting and idle slots write song -1 into the ring row (the plain form writes song[s] as it is, and no
//             slot with song < 0 ever takes a song there).
// The plain form has ctl = {tokens advanced, songs assigned, songs finished} and never touches a fourth element.
#include "cwlt_common.h"

namespace cwlt {

// One block per CU-sized share of a slot's state: every block walks the fresh flags (a ballot per 64 slots) and, for
// each flagged slot, copies its 1/gridDim share of the source.  The slot layout is DecodeSession._state: per layer
// S of all slots ([slots][s4] float4) then Z of all slots ([slots][z4] float4); the source is the same for one slot,
// or (BANK) for `bank` entries with logits rows ld_src_logits apart.  bank, ld_src_logits and song are BANK's alone.
template <bool BANK>
__global__ __launch_bounds__(256) void stream_refill_kernel(float4* __restrict__ state, const float4* __restrict__ src,
                                                            long bank, long slots, int n_layer, long s4, long z4,
                                                            float* __restrict__ logits,
                                                            const float* __restrict__ src_logits, long n_logits,
                                                            long ld_logits, long ld_src_logits,
                                                            const int64_t* __restrict__ fresh,
                                                            const int64_t* __restrict__ song) {
    __shared__ unsigned long long mask_s[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long per = s4 + z4, total = (long)n_layer * per;
    const long first = (long)blockIdx.x * blockDim.x + tid, stride = (long)gridDim.x * blockDim.x;
    for (long base = 0; base < slots; base += 256) {
        const long s = base + tid;
        const bool f = s < slots && fresh[s] != 0 && (!BANK || song[s] >= 0);
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
                const long e = BANK ? song[slot] % bank : 0;
                for (long j = first; j < total; j += stride) {
                    const long layer = j / per, r = j - layer * per;
                    const long d = layer * slots * per + (r < s4 ? slot * s4 + r : slots * s4 + slot * z4 + (r - s4));
                    const long from =
                        BANK ? layer * bank * per + (r < s4 ? e * s4 + r : bank * s4 + e * z4 + (r - s4)) : j;
                    state[d] = src[from];
                }
                const float* row = BANK ? src_logits + e * ld_src_logits : src_logits;
                for (long j = first; j < n_logits; j += stride) logits[slot * ld_logits + j] = row[j];
            }
        }
    }
}

// Where a newly assigned slot's bar0 and cap come from: two scalars, or (BANK) the new song's bank entry, the cap kept
// per slot.
template <bool BANK>
struct StreamStart {
    long bar0, cap;
};
template <>
struct StreamStart<true> {
    const int64_t* bar0;                             // [bank]
    const int64_t* cap;                              // [bank]
    long bank;
    int64_t* slot_cap;                               // [slots]
};

__device__ inline long cap_of(const StreamStart<false>& st, long) { return st.cap; }
__device__ inline long cap_of(const StreamStart<true>& st, long s) { return st.slot_cap[s]; }
// Slot s takes song idx -> the bar count it starts from.
__device__ inline long start(const StreamStart<false>& st, long, long) { return st.bar0; }
__device__ inline long start(const StreamStart<true>& st, long idx, long s) {
    const long e = idx % st.bank;
    st.slot_cap[s] = st.cap[e];
    return st.bar0[e];
}

// One workgroup: slots in chunks of blockDim.  The candidates for a new song -- the slots whose song ended on this token
// and (BANK) the slots already waiting -- are ranked in slot order by a ballot prefix per wave and the wave totals; the
// first `limit - assigned` of them take songs, the rest wait (BANK, while songs remain) or go idle.
template <bool BANK>
__global__ __launch_bounds__(1024) void stream_advance_kernel(
    const int64_t* __restrict__ tokens, int n_attr, long slots, int bar_attr, const int* __restrict__ bar_mask,
    int bar_classes, long bar_cond, StreamStart<BANK> st, long n_songs, int64_t* __restrict__ song,
    int64_t* __restrict__ pos, int64_t* __restrict__ bar, int64_t* __restrict__ fresh, int64_t* __restrict__ ctl,
    int64_t* __restrict__ ring, long ring_rows) {
    __shared__ int wave_n[16], wave_e[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n_wave = blockDim.x >> 6;
    const long t = ctl[0], assigned = ctl[1];
    long limit = n_songs;                            // song indices below this may be handed out
    if (BANK && ctl[3] < limit) limit = ctl[3];
    const long row = t % ring_rows;
    long carry = 0, carry_e = 0;                     // candidates / (BANK) ended slots before this chunk
    for (long base = 0; base < slots; base += blockDim.x) {
        const long s = base + tid;
        const bool active = s < slots;
        int ended = 0, cand = 0;
        if (active) {
            const long sg = song[s];
            int64_t* out = ring + (row * slots + s) * (n_attr + 2);
            out[0] = BANK && sg < 0 ? -1 : sg;
            for (int a = 0; a < n_attr; ++a) out[1 + a] = tokens[s * n_attr + a];
            if (sg >= 0) {
                const long p = pos[s];
                long b = bar[s];
                const long tk = tokens[s * n_attr + bar_attr];
                if (tk >= 0 && tk < bar_classes && bar_mask[tk]) ++b;
                ended = (b >= bar_cond || p + 1 >= cap_of(st, s)) ? 1 : 0;
                pos[s] = p + 1;
                bar[s] = b;
            }
            out[n_attr + 1] = ended;
            cand = (ended || (BANK && sg == -2)) ? 1 : 0;
        }
        const unsigned long long m = __ballot(cand != 0);
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (BANK) {                                  // plain: the candidates are the ended slots
            const unsigned long long me = __ballot(ended != 0);
            if (lane == 0) wave_e[w] = __popcll(me);
        }
        if (lane == 0) wave_n[w] = __popcll(m);
        __syncthreads();
        int before = 0, chunk_n = 0, chunk_e = 0;
        for (int q = 0; q < n_wave; ++q) {
            before += q < w ? wave_n[q] : 0;
            chunk_n += wave_n[q];
            if (BANK) chunk_e += wave_e[q];
        }
        __syncthreads();                             // wave_n / wave_e are rewritten by the next chunk
        if (active) {
            const long idx = assigned + carry + before + rank;
            const bool take = cand && idx < limit;
            if (take) {
                song[s] = idx;
                pos[s] = 0;
                bar[s] = start(st, idx, s);
            } else if (cand) {
                song[s] = BANK && idx < n_songs ? -2 : -1;   // wait for the song's entry, or idle: none left
            }
            fresh[s] = BANK ? take : cand;           // plain: an idle slot is refilled once, then stepped and ignored
        }
        carry += chunk_n;
        if (BANK) carry_e += chunk_e;
    }
    if (tid == 0) {
        const long room = limit > assigned ? limit - assigned : 0;   // BANK: songs the gate lets out
        ctl[0] = t + 1;
        const long next = assigned + (BANK && carry > room ? room : carry);
        ctl[1] = !BANK && next > n_songs ? n_songs : next;
        ctl[2] = ctl[2] + (BANK ? carry_e : carry);    // plain: the candidates are the ended slots
    }
}

// The checks and the launch the two refill entries share (bank = 1, song = nullptr in the plain form).
template <bool BANK>
static int stream_refill(float* state, const float* src, int64_t bank, int n_layer, int64_t s_floats,
                         int64_t z_floats, float* logits, const float* src_logits, int64_t n_logits,
                         int64_t ld_logits, int64_t ld_src_logits, const int64_t* fresh, const int64_t* song,
                         int64_t slots, void* stream) {
    if (!state || !src || !logits || !src_logits || !fresh) return CWLT_ERR_ARG;
    if (n_layer < 1 || slots < 1 || s_floats < 4 || z_floats < 4 || s_floats % 4 || z_floats % 4 || n_logits < 1 ||
        ld_logits < n_logits)
        return CWLT_ERR_ARG;
    if (((uintptr_t)state | (uintptr_t)src) % 16) return CWLT_ERR_ARG;
    const long total = (long)n_layer * ((s_floats + z_floats) / 4);
    long blocks = (total + 255) / 256;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(stream_refill_kernel<BANK>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (float4*)state, (const float4*)src, (long)bank, (long)slots, n_layer, (long)s_floats / 4,
                       (long)z_floats / 4, logits, src_logits, (long)n_logits, (long)ld_logits, (long)ld_src_logits,
                       fresh, song);
    return (int)hipGetLastError();
}

// The checks and the launch the two advance entries share.
template <bool BANK>
static int stream_advance(const int64_t* tokens, int n_attr, int64_t slots, int bar_attr, const int* bar_mask,
                          int bar_classes, int64_t bar_cond, StreamStart<BANK> st, int64_t n_songs, int64_t* song,
                          int64_t* pos, int64_t* bar, int64_t* fresh, int64_t* ctl, int64_t* ring, int64_t ring_rows,
                          void* stream) {
    if (!tokens || !bar_mask || !song || !pos || !bar || !fresh || !ctl || !ring) return CWLT_ERR_ARG;
    if (n_attr < 1 || n_attr > 8 || bar_attr < 0 || bar_attr >= n_attr || bar_classes < 1 || slots < 1 ||
        ring_rows < 1 || n_songs < 0 || n_songs > (1L << 20))
        return CWLT_ERR_ARG;
    hipLaunchKernelGGL(stream_advance_kernel<BANK>, dim3(1), dim3(1024), 0, (hipStream_t)stream, tokens, n_attr,
                       (long)slots, bar_attr, bar_mask, bar_classes, (long)bar_cond, st, (long)n_songs, song, pos, bar,
                       fresh, ctl, ring, (long)ring_rows);
    return (int)hipGetLastError();
}

}  // namespace cwlt

extern "C" int cwlt_stream_refill(float* state, const float* snap_state, int n_layer, int64_t s_floats,
                                  int64_t z_floats, float* logits, const float* snap_logits, int64_t n_logits,
                                  int64_t ld_logits, const int64_t* fresh, int64_t slots, void* stream) {
    return cwlt::stream_refill<false>(state, snap_state, 1, n_layer, s_floats, z_floats, logits, snap_logits, n_logits,
                                      ld_logits, n_logits, fresh, nullptr, slots, stream);
}

extern "C" int cwlt_stream_advance(const int64_t* tokens, int n_attr, int64_t slots, int bar_attr, const int* bar_mask,
                                   int bar_classes, int64_t bar_cond, int64_t bar0, int64_t cap, int64_t n_songs,
                                   int64_t* song, int64_t* pos, int64_t* bar, int64_t* fresh, int64_t* ctl,
                                   int64_t* ring, int64_t ring_rows, void* stream) {
    if (cap < 1 || bar0 >= bar_cond) return CWLT_ERR_ARG;
    return cwlt::stream_advance<false>(tokens, n_attr, slots, bar_attr, bar_mask, bar_classes, bar_cond,
                                       {(long)bar0, (long)cap}, n_songs, song, pos, bar, fresh, ctl, ring, ring_rows,
                                       stream);
}

extern "C" int cwlt_stream_refill_bank(float* state, const float* bank_state, int64_t bank, int n_layer,
                                       int64_t s_floats, int64_t z_floats, float* logits, const float* bank_logits,
                                       int64_t n_logits, int64_t ld_logits, int64_t ld_bank_logits,
                                       const int64_t* fresh, const int64_t* song, int64_t slots, void* stream) {
    if (!song || bank < 1 || ld_bank_logits < n_logits) return CWLT_ERR_ARG;
    return cwlt::stream_refill<true>(state, bank_state, bank, n_layer, s_floats, z_floats, logits, bank_logits,
                                     n_logits, ld_logits, ld_bank_logits, fresh, song, slots, stream);
}

extern "C" int cwlt_stream_advance_bank(const int64_t* tokens, int n_attr, int64_t slots, int bar_attr,
                                        const int* bar_mask, int bar_classes, int64_t bar_cond,
                                        const int64_t* bank_bar0, const int64_t* bank_cap, int64_t bank,
                                        int64_t n_songs, int64_t* song, int64_t* pos, int64_t* bar, int64_t* cap,
                                        int64_t* fresh, int64_t* ctl, int64_t* ring, int64_t ring_rows,
                                        void* stream) {
    if (!bank_bar0 || !bank_cap || !cap || bank < 1 || bar_cond < 1) return CWLT_ERR_ARG;
    return cwlt::stream_advance<true>(tokens, n_attr, slots, bar_attr, bar_mask, bar_classes, bar_cond,
                                      {bank_bar0, bank_cap, (long)bank, cap}, n_songs, song, pos, bar, fresh, ctl,
                                      ring, ring_rows, stream);
}
