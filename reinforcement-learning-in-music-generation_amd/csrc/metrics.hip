// Song metrics (generation.song_metrics, generation.MetricReward): what the compound-word and
// Jazz-Transformer papers report about generated songs -- pitch-class entropy over 1 and 4 bars, grooving similarity --
// and a few rule-based measures (notes inside the sounding chord, pitch range, empty bars), computed from token rows on
// the device and, with a weight per measure, folded into one reward per song.
//
// One entry point, cwlt_song_metrics; its definitions are in include/cwlt.h and every output is bitwise
// sampling.song_metrics_f32.  One song per group of threads; the rows of a song are taken in strides of the group:
//   * the bar slot of a row is a prefix count of Bar rows; its beat and its chord are the value of the last setter at or
//     before it.  Inside a wave these are ballots (a prefix popcount; the highest set bit at or below the lane, then one
//     cross-lane read of that lane's value), across the waves of a group one summary per wave in LDS, and from stride to
//     stride a carry every thread keeps;
//   * per-slot pitch-class histograms, beat masks and note counts are LDS integer atomics, so their order is irrelevant;
//   * everything in floating point is computed per slot in parallel (an entropy reads 12 counts and 13 table entries) and
//     then summed by one thread in slot order: the order the definitions fix.
// Two group sizes: a wave per song, four songs to a 256-thread workgroup and no workgroup barrier (the reward windows:
// 50 rows, 51 slots at most), and 256 threads per song beyond METRIC_WAVE_ROWS rows or METRIC_WAVE_SLOTS slots.  Both are
// the same template; the results are integers and floats in a fixed order, so the choice cannot show.
// No host synchronisation, no allocation, no cross-workgroup communication.
#include "cwlt_common.h"

namespace cwlt {

constexpr int METRIC_F = 11;
constexpr int METRIC_WAVE_ROWS = 128, METRIC_WAVE_SLOTS = 64, METRIC_MAX_SLOTS = 512;
constexpr long METRIC_MAX_ROWS = (1L << 24) - 1;        // a note count is exact as a float

struct MetricArgs {
    const int64_t* tok;
    const int64_t* mask;
    const int32_t* lengths;
    long N, L;
    int A, bar_attr, pitch_attr, chord_attr;
    const int32_t *order, *pitch, *chord;
    int n_order, n_pitch, n_chord, Q;
    const float* xlog2x;
    int max_bars;
    float* feat;
    const float* weights;
    float* reward;
    int32_t* bars;
    int32_t* hist;
    int64_t* groove;
};

// The LDS of one song: CAP slots of 12 counts + a 64-bit beat mask + a note count (60 bytes), the two per-slot
// entropies with the 4-bar runs' note counts (12 bytes), and the song's scalars.
template <int CAP>
struct MetricLds {
    int hist[CAP * 12];
    unsigned long long groove[CAP];
    int cnt[CAP];
    float e1[CAP];
    float e4[CAP];
    int n4[CAP];
    unsigned long long pset[2];
    int tot[12];
    int notes, n_c, n_h, pmin, pmax, empty;
    unsigned int xor_bits;
};

// What a wave knows after one stride: its Bar rows, the last beat and chord it set, and whether it has a live row in
// front of its first Bar row.
struct MetricWave {
    int bars, beat_set, beat, chord_set, chord, head;
};

// Orders the LDS traffic of a group.  A wave on its own issues its LDS operations in order: the fence keeps the compiler
// from moving them and waits for the ones in flight; the wave form has no workgroup barrier.
template <int WAVES>
__device__ __forceinline__ void metric_sync() {
    if (WAVES > 1) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
}

// (T[n] - (((0 + T[c0]) + T[c1]) + ... + T[c11])) / n, every operation rounded on its own; 0 for n = 0.
__device__ inline float metric_entropy(const int (&c)[12], const float* __restrict__ T) {
#pragma clang fp contract(off)
    int n = 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) n += c[k];
    if (n == 0) return 0.f;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 12; ++k) s += T[c[k]];
    return (T[n] - s) / (float)n;
}

__device__ inline float metric_ratio(int num, int den) {
#pragma clang fp contract(off)
    return den ? (float)num / (float)den : 0.f;
}

template <int WAVES, int SONGS, int CAP>
__global__ __launch_bounds__(256) void song_metrics_kernel(const MetricArgs a) {
    constexpr int T = 64 * WAVES;
    static_assert(WAVES * SONGS == 4, "256 threads");
    __shared__ MetricLds<CAP> lds[SONGS];
    __shared__ MetricWave xw[2][WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int sub = WAVES == 1 ? wave : 0;
    const int t = WAVES == 1 ? lane : (int)threadIdx.x;
    const long n = (long)blockIdx.x * SONGS + sub;
    if (n >= a.N) return;                               // a whole wave of the wave form; never in the block form
    MetricLds<CAP>& s = lds[sub];
    const int MB = a.max_bars;                          // <= CAP: the launcher's choice of the form

    for (int i = t; i < MB * 12; i += T) s.hist[i] = 0;
    for (int i = t; i < MB; i += T) {
        s.groove[i] = 0ull;
        s.cnt[i] = 0;
    }
    if (t < 12) s.tot[t] = 0;
    if (t == 0) {
        s.pset[0] = s.pset[1] = 0ull;
        s.notes = s.n_c = s.n_h = s.empty = 0;
        s.pmin = 128;
        s.pmax = -1;
        s.xor_bits = 0u;
    }
    metric_sync<WAVES>();

    long len = a.L;
    if (a.lengths) {
        const long l = a.lengths[n];
        len = l < 0 ? 0 : (l < a.L ? l : a.L);
    }
    const int64_t* rows = a.tok + n * a.L * a.A;
    const int64_t* live_row = a.mask ? a.mask + n * a.L : nullptr;
    int c_bars = 0, c_beat = -1, c_chord = 0, c_head = 0;                   // the carry: the same in every thread
    int my_notes = 0, my_nc = 0, my_nh = 0, my_min = 128, my_max = -1;
    unsigned long long my_p0 = 0ull, my_p1 = 0ull;
    const unsigned long long le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);      // the lanes at or below mine

    int parity = 0;
    for (long base = 0; base < len; base += T, parity ^= 1) {
        const long i = base + t;
        bool live = i < len;
        if (live && live_row) live = live_row[i] != 0;
        int o = -3, ch = -1, pit = -1;
        if (live) {
            const int64_t* r = rows + i * a.A;
            const int64_t cb = r[a.bar_attr], cp = r[a.pitch_attr], cc = a.chord_attr >= 0 ? r[a.chord_attr] : 0;
            const bool inside = cb >= 0 && cb < a.n_order && cp >= 0 && cp < a.n_pitch &&
                                (a.chord_attr < 0 || (cc >= 0 && cc < a.n_chord));
            if (inside) {
                o = a.order[cb];
                pit = a.pitch[cp];
                ch = a.chord_attr >= 0 ? a.chord[cc] : -1;
            }
        }
        const bool is_bar = o == -1, sets_beat = o >= -1, sets_chord = o >= 0 && ch >= 0;
        const bool is_note = o == -2 && pit >= 0 && pit < 128;

        // inside the wave
        const unsigned long long b_bar = __ballot(is_bar), b_beat = __ballot(sets_beat);
        const unsigned long long b_chord = __ballot(sets_chord), b_live = __ballot(live);
        const int w_bars = __popcll(b_bar & le);
        const unsigned long long m_beat = b_beat & le, m_chord = b_chord & le;
        const int beat_v = __shfl(o, m_beat ? 63 - __clzll(m_beat) : lane, 64);
        const int chord_v = __shfl(ch, m_chord ? 63 - __clzll(m_chord) : lane, 64);
        MetricWave mine;
        mine.bars = __popcll(b_bar);
        mine.beat_set = b_beat != 0ull;
        mine.beat = __builtin_amdgcn_readlane(beat_v, 63);
        mine.chord_set = b_chord != 0ull;
        mine.chord = __builtin_amdgcn_readlane(chord_v, 63);
        mine.head = (b_live & (b_bar ? (b_bar & (0ull - b_bar)) - 1ull : ~0ull)) != 0ull;

        // across the waves, and the carry
        int p_bars = c_bars, p_beat = c_beat, p_chord = c_chord;
        if (WAVES > 1) {
            if (lane == 0) xw[parity][wave] = mine;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                const MetricWave x = xw[parity][w];
                if (w == wave) {
                    p_bars = c_bars;
                    p_beat = c_beat;
                    p_chord = c_chord;
                }
                if (c_bars == 0 && x.head) c_head = 1;
                c_bars += x.bars;
                if (x.beat_set) c_beat = x.beat;
                if (x.chord_set) c_chord = x.chord;
            }
        } else {
            if (c_bars == 0 && mine.head) c_head = 1;
            c_bars += mine.bars;
            if (mine.beat_set) c_beat = mine.beat;
            if (mine.chord_set) c_chord = mine.chord;
        }
        const int slot = p_bars + w_bars;
        const int beat = m_beat ? beat_v : p_beat;
        const int chord = m_chord ? chord_v : p_chord;

        if (is_note && slot < MB) {
            const int pc = pit % 12;
            atomicAdd(&s.hist[slot * 12 + pc], 1);
            atomicAdd(&s.cnt[slot], 1);
            if (beat >= 0 && beat < 64) atomicOr(&s.groove[slot], 1ull << beat);
            ++my_notes;
            if (chord != 0) {
                ++my_nc;
                my_nh += (chord >> pc) & 1;
            }
            my_min = pit < my_min ? pit : my_min;
            my_max = pit > my_max ? pit : my_max;
            if (pit < 64) my_p0 |= 1ull << pit;
            else my_p1 |= 1ull << (pit - 64);
        }
    }
    if (my_notes) {
        atomicAdd(&s.notes, my_notes);
        atomicAdd(&s.n_c, my_nc);
        atomicAdd(&s.n_h, my_nh);
        atomicMin(&s.pmin, my_min);
        atomicMax(&s.pmax, my_max);
        if (my_p0) atomicOr(&s.pset[0], my_p0);
        if (my_p1) atomicOr(&s.pset[1], my_p1);
    }
    metric_sync<WAVES>();

    // The existing slots are first .. c_bars (slot 0 only with a live row in front of the first Bar row); the ones kept
    // are those below max_bars.
    const int first = c_head ? 0 : 1;
    const int B = c_bars + 1 - first;
    const int hi = c_bars + 1 < MB ? c_bars + 1 : MB;
    for (int sl = first + t; sl < hi; sl += T) {
        int c[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) c[k] = s.hist[sl * 12 + k];
        s.e1[sl] = metric_entropy(c, a.xlog2x);
        if (s.cnt[sl] == 0) atomicAdd(&s.empty, 1);
        if (sl + 3 < hi) {
            int n4 = 0;
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                c[k] += s.hist[(sl + 1) * 12 + k] + s.hist[(sl + 2) * 12 + k] + s.hist[(sl + 3) * 12 + k];
                n4 += c[k];
            }
            s.n4[sl] = n4;
            s.e4[sl] = metric_entropy(c, a.xlog2x);
        }
        const unsigned long long g = s.groove[sl];
        unsigned int x = 0u;
        for (int j = sl + 1; j < hi; ++j) x += (unsigned int)__popcll(g ^ s.groove[j]);
        if (x) atomicAdd(&s.xor_bits, x);
    }
    if (t < 12) {
        int c = 0;
        for (int sl = first; sl < hi; ++sl) c += s.hist[sl * 12 + t];
        s.tot[t] = c;
    }
    metric_sync<WAVES>();

    if (t == 0) {
#pragma clang fp contract(off)
        float f[METRIC_F];
        const int Bk = hi > first ? hi - first : 0;
        float sum = 0.f;
        int count = 0;
        for (int sl = first; sl < hi; ++sl)
            if (s.cnt[sl] > 0) {
                sum += s.e1[sl];
                ++count;
            }
        f[2] = count ? sum / (float)count : 0.f;
        sum = 0.f;
        count = 0;
        for (int sl = first; sl + 3 < hi; ++sl)
            if (s.n4[sl] > 0) {
                sum += s.e4[sl];
                ++count;
            }
        f[3] = count ? sum / (float)count : 0.f;
        int c[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) c[k] = s.tot[k];
        f[4] = metric_entropy(c, a.xlog2x);
        const int P = Bk * (Bk - 1) / 2;
        f[5] = P ? 1.0f - (float)s.xor_bits / (float)(P * a.Q) : 0.f;
        f[0] = (float)s.notes;
        f[1] = (float)B;
        f[6] = metric_ratio(s.n_h, s.n_c);
        f[7] = s.notes ? (float)(s.pmax - s.pmin) : 0.f;
        f[8] = (float)(__popcll(s.pset[0]) + __popcll(s.pset[1]));
        f[9] = metric_ratio(s.notes, Bk);
        f[10] = metric_ratio(s.empty, Bk);
        float* out = a.feat + n * METRIC_F;
#pragma unroll
        for (int k = 0; k < METRIC_F; ++k) out[k] = f[k];
        if (a.reward) {
            float r = 0.f;
#pragma unroll
            for (int k = 0; k < METRIC_F; ++k) {
                const float m = a.weights[k] * f[k];
                r = r + m;
            }
            a.reward[n] = r;
        }
        if (a.bars) a.bars[n] = B;
    }
    if (a.hist) {
        int32_t* out = a.hist + n * MB * 12;
        for (int i = t; i < MB * 12; i += T) out[i] = s.hist[i];
    }
    if (a.groove) {
        int64_t* out = a.groove + n * MB;
        for (int i = t; i < MB; i += T) out[i] = (int64_t)s.groove[i];
    }
}

}  // namespace cwlt

extern "C" int cwlt_song_metrics(const int64_t* tok, const int64_t* mask, const int32_t* lengths, int64_t N, int64_t L,
                                 int n_attr, int bar_attr, int pitch_attr, int chord_attr, const int32_t* order,
                                 int n_order, const int32_t* pitch, int n_pitch, const int32_t* chord, int n_chord, int Q,
                                 const float* xlog2x, int64_t n_table, int max_bars, float* feat, const float* weights,
                                 float* reward, int32_t* bars, int32_t* hist, int64_t* groove, void* stream) {
    using namespace cwlt;
    if (!tok || !order || !pitch || !xlog2x || !feat) return CWLT_ERR_ARG;
    if (N < 1 || N > (1L << 24) || L < 1 || L > METRIC_MAX_ROWS || n_attr < 1 || n_attr > 8) return CWLT_ERR_ARG;
    if (bar_attr < 0 || bar_attr >= n_attr || pitch_attr < 0 || pitch_attr >= n_attr || chord_attr < -1 ||
        chord_attr >= n_attr)
        return CWLT_ERR_ARG;
    if (n_order < 1 || n_pitch < 1 || (chord_attr >= 0 && (!chord || n_chord < 1))) return CWLT_ERR_ARG;
    if (Q < 1 || Q > 64 || max_bars < 1 || max_bars > METRIC_MAX_SLOTS || n_table < L + 1) return CWLT_ERR_ARG;
    if (reward && !weights) return CWLT_ERR_ARG;
    MetricArgs a;
    a.tok = tok, a.mask = mask, a.lengths = lengths;
    a.N = (long)N, a.L = (long)L;
    a.A = n_attr, a.bar_attr = bar_attr, a.pitch_attr = pitch_attr, a.chord_attr = chord_attr;
    a.order = order, a.pitch = pitch, a.chord = chord;
    a.n_order = n_order, a.n_pitch = n_pitch, a.n_chord = n_chord, a.Q = Q;
    a.xlog2x = xlog2x;
    a.max_bars = max_bars;
    a.feat = feat, a.weights = weights, a.reward = reward, a.bars = bars, a.hist = hist, a.groove = groove;
    if (L <= METRIC_WAVE_ROWS && max_bars <= METRIC_WAVE_SLOTS)
        hipLaunchKernelGGL((song_metrics_kernel<1, 4, METRIC_WAVE_SLOTS>), dim3((unsigned)((N + 3) / 4)), dim3(256), 0,
                           (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((song_metrics_kernel<4, 1, METRIC_MAX_SLOTS>), dim3((unsigned)N), dim3(256), 0,
                           (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
