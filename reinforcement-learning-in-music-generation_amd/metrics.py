"""Song metrics on the device, and as rewards for particle generation.

`SongMetricSpec` compiles a compound-word vocabulary into the tables cwlt_song_metrics reads; `song_metrics` evaluates
a set of songs (pitch-class entropy over 1 and 4 bars, grooving similarity, notes inside the sounding chord, ...);
`MetricReward` is a rule-based reward callable for generate_particles(reward=): a weighted sum of the same measures
over each particle's window, one launch on the current stream.  The definitions are restated in numpy as
sampling.song_metrics_f32, which the kernel matches bit for bit.
"""
import numpy as np
import torch

from . import ops
from .draw_plan import Grammar

METRICS = ("n_notes", "n_bars", "h1", "h4", "h_all", "groove", "in_chord", "pitch_range", "distinct_pitches",
           "notes_per_bar", "empty_bars")
MAX_BARS = 512
MAX_BEATS = 64

CHORD_ROOTS = ("C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B")
CHORD_QUALITIES = {"M": (0, 4, 7), "m": (0, 3, 7), "o": (0, 3, 6), "+": (0, 4, 8), "7": (0, 4, 7, 10),
                   "M7": (0, 4, 7, 11), "m7": (0, 3, 7, 10), "o7": (0, 3, 6, 9), "/o7": (0, 3, 6, 10),
                   "sus2": (0, 2, 7), "sus4": (0, 5, 7)}


def _chord_mask(name):
    """The 12-bit pitch-class mask of a chord name "<root>_<quality>", -1 for CONTI, 0 for N_N; None if it is neither."""
    if name == "CONTI":
        return -1
    if name == "N_N":
        return 0
    if not isinstance(name, str) or "_" not in name:
        return None
    root, quality = name.split("_", 1)
    if root not in CHORD_ROOTS or quality not in CHORD_QUALITIES:
        return None
    r = CHORD_ROOTS.index(root)
    return sum(1 << ((r + i) % 12) for i in CHORD_QUALITIES[quality])


class SongMetricSpec:
    """A CP vocabulary compiled into the four tables of cwlt_song_metrics.
    order: Grammar's table of `bar_attr` (-2 class 0, -1 "Bar", k Beat_<k>), with Grammar's refusals; Q = max k + 1.
    pitch: per class of `pitch_attr` the MIDI pitch int(name.split("_")[-1]) (midi.words_to_events' parse), -1 for
      class 0; pitches={class id: midi} overrides.
    chord: per class of `chord_attr` -1 for class 0 and "CONTI" (keep the current chord), 0 for "N_N" (no chord), else
      the 12-bit pitch-class mask of "<root>_<quality>" (roots C C# D ... B; qualities M m o + 7 M7 m7 o7 /o7 sus2 sus4,
      data.synthetic_cp_vocabulary's spellings); chords={class id: pitch classes} overrides.  chord_attr=None turns the
      chord feature off (in_chord is 0).
    xlog2x(n): T[c] = float32(c log2 c) for c < n, computed in float64 and rounded once.
    Refused (ValueError): unknown attributes, what Grammar refuses, no beat class or Q > 64, a pitch class that does
    not parse or lies outside 0..127, a chord class that is none of the above, overrides for class ids outside the
    attribute, max_bars outside 1..512."""

    def __init__(self, word2event, bar_attr="bar-beat", pitch_attr="pitch", chord_attr="chord", pitches=None,
                 chords=None, max_bars=MAX_BARS):
        self.keys = list(word2event.keys())
        self.n_class = [len(word2event[k]) for k in self.keys]
        for name in (pitch_attr,) + (() if chord_attr is None else (chord_attr,)):
            if name not in self.keys:
                raise ValueError("unknown attribute %r (attributes: %s)" % (name, ", ".join(map(str, self.keys))))
        self.order = Grammar(word2event, bar_attr=bar_attr, metrical=(), note=()).order.astype(np.int32)
        self.bar_attr = self.keys.index(bar_attr)
        self.pitch_attr = self.keys.index(pitch_attr)
        self.chord_attr = -1 if chord_attr is None else self.keys.index(chord_attr)
        if int(self.order.max()) < 0:
            raise ValueError("%s has no beat class (Beat_<k>)" % (bar_attr,))
        self.Q = int(self.order.max()) + 1
        if self.Q > MAX_BEATS:
            raise ValueError("%s: beat index %d, at most %d beats per bar are counted" % (bar_attr, self.Q - 1,
                                                                                         MAX_BEATS))
        self.max_bars = int(max_bars)
        if not 1 <= self.max_bars <= MAX_BARS:
            raise ValueError("max_bars must lie in 1..%d, got %r" % (MAX_BARS, max_bars))

        names, n = word2event[pitch_attr], self.n_class[self.pitch_attr]
        over = self._overrides("pitches", pitches, n)
        self.pitch = np.full(n, -1, dtype=np.int32)
        for c in range(1, n):
            if c in over:
                p = int(over[c])
            else:
                try:
                    p = int(str(names[c]).split("_")[-1])
                except ValueError:
                    raise ValueError("%s class %d (%r) does not end in a MIDI pitch: pass pitches={class id: midi}"
                                     % (pitch_attr, c, names[c])) from None
            if not 0 <= p <= 127:
                raise ValueError("%s class %d (%r): pitch %d outside 0..127" % (pitch_attr, c, names[c], p))
            self.pitch[c] = p

        self.chord = None
        if chord_attr is not None:
            names, n = word2event[chord_attr], self.n_class[self.chord_attr]
            over = self._overrides("chords", chords, n)
            self.chord = np.full(n, -1, dtype=np.int32)
            for c in range(1, n):
                if c in over:
                    try:
                        pcs = [int(p) for p in over[c]]
                    except TypeError:
                        raise ValueError("chords[%d] must be an iterable of pitch classes" % c) from None
                    if any(not 0 <= p <= 11 for p in pcs):
                        raise ValueError("chords[%d]: pitch classes lie in 0..11, got %s" % (c, pcs))
                    m = sum(1 << p for p in set(pcs))
                else:
                    m = _chord_mask(names[c])
                    if m is None:
                        raise ValueError("%s class %d (%r) is neither CONTI, N_N nor <root>_<quality>: pass "
                                         "chords={class id: pitch classes}" % (chord_attr, c, names[c]))
                self.chord[c] = m
        elif chords is not None:
            raise ValueError("chords= given with chord_attr=None")
        self._device = {}

    @staticmethod
    def _overrides(what, table, n):
        table = {} if table is None else {int(c): v for c, v in dict(table).items()}
        for c in table:
            if not 1 <= c < n:
                raise ValueError("%s: class id %d outside 1..%d" % (what, c, n - 1))
        return table

    @staticmethod
    def xlog2x(n_table):
        """T (n_table,) float32: T[c] = c log2 c in float64, rounded once; T[0] = T[1] = 0."""
        c = np.arange(int(n_table), dtype=np.float64)
        return (c * np.log2(np.maximum(c, 1.0))).astype(np.float32)

    def tables(self, device, n_table):
        """The device tables -> (order, pitch, chord or None, xlog2x with at least n_table entries), cached per device;
        the xlog2x table grows by doubling, so a loop of one shape uploads once."""
        key = str(torch.device(device))
        have = self._device.get(key)
        if have is None or have[3].numel() < int(n_table):
            size = max(int(n_table), 64, 0 if have is None else 2 * have[3].numel())
            put = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
            have = (put(self.order), put(self.pitch), put(self.chord), put(self.xlog2x(size)))
            self._device[key] = have
        return have

    @property
    def attrs(self):
        return (self.bar_attr, self.pitch_attr, self.chord_attr)


def _as_spec(word2event_or_spec):
    return word2event_or_spec if isinstance(word2event_or_spec, SongMetricSpec) else SongMetricSpec(word2event_or_spec)


def song_metrics(word2event_or_spec, songs, mask=None, device=None):
    """The measures of METRICS for a set of songs, computed on the GPU (cwlt_song_metrics, one launch).
    songs: a list of (L_i, A) integer arrays, or one (N, L, A) array; mask: (N, L) with the array form only (nonzero:
    the row counts).  A list is padded to its longest song and the lengths go to the kernel.
    -> a dict: every name of METRICS -> (N,) float32 numpy; "bars" (N,) int32, the songs' bar slots; "hist"
    (N, max_bars, 12) int32 and "groove_masks" (N, max_bars) int64 ("groove" is the measure), per slot the pitch-class
    counts and the beats that carry a note (slot s >= 1 the s-th Bar row's bar, slot 0 what precedes the first).  max_bars is sized from the songs on
    the host: the most Bar rows of a song + 1; more than 512 is refused (cut the songs)."""
    spec = _as_spec(word2event_or_spec)
    A = len(spec.keys)
    lengths = None
    if isinstance(songs, (list, tuple)):
        if mask is not None:
            raise ValueError("mask goes with an (N, L, A) array; a list of songs carries its own lengths")
        rows = [np.asarray(s, dtype=np.int64).reshape(-1, A) for s in songs]
        if not rows:
            raise ValueError("song_metrics needs at least one song")
        lengths = np.array([len(r) for r in rows], dtype=np.int32)
        tok = np.zeros((len(rows), max(1, int(lengths.max())), A), dtype=np.int64)
        for i, r in enumerate(rows):
            tok[i, :len(r)] = r
    else:
        tok = np.ascontiguousarray(np.asarray(songs, dtype=np.int64))
        if tok.ndim != 3 or tok.shape[2] != A or tok.shape[0] < 1 or tok.shape[1] < 1:
            raise ValueError("songs must be a list of (L_i, %d) arrays or one (N, L, %d) array, got shape %s"
                             % (A, A, tok.shape))
    N, L, _ = tok.shape
    if mask is not None:
        mask = np.ascontiguousarray(np.asarray(mask) != 0).astype(np.int64)
        if mask.shape != (N, L):
            raise ValueError("mask must be (%d, %d), got %s" % (N, L, mask.shape))
    cb = tok[:, :, spec.bar_attr]
    is_bar = (cb >= 0) & (cb < len(spec.order)) & (spec.order[np.clip(cb, 0, len(spec.order) - 1)] == -1)
    max_bars = int(is_bar.sum(axis=1).max()) + 1
    if max_bars > MAX_BARS:
        raise ValueError("a song has %d Bar rows: at most %d bar slots are counted (cut the songs)"
                         % (max_bars - 1, MAX_BARS))
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("song_metrics runs on a GPU: the cwlt hot path has no CPU implementation (device=%r)" % (device,))
    order, pitch, chord, table = spec.tables(dev, L + 1)
    put = lambda a: None if a is None else torch.from_numpy(a).to(dev)                              # noqa: E731
    feat = torch.empty(N, len(METRICS), dtype=torch.float32, device=dev)
    bars = torch.empty(N, dtype=torch.int32, device=dev)
    hist = torch.empty(N, max_bars, 12, dtype=torch.int32, device=dev)
    groove = torch.empty(N, max_bars, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        ops.song_metrics(put(tok), put(mask), put(lengths), spec.attrs, order, pitch, chord, spec.Q, table, max_bars,
                         feat, bars=bars, hist=hist, groove=groove)
    f = feat.cpu().numpy()
    out = {name: f[:, i].copy() for i, name in enumerate(METRICS)}
    out.update(bars=bars.cpu().numpy(), hist=hist.cpu().numpy(), groove_masks=groove.cpu().numpy())
    return out


class MetricReward:
    """A rule-based reward callable for generate_particles(reward=) and generate(particles=, reward=): a weighted sum
    of the song measures of METRICS over each particle's window, e.g. MetricReward(word2event, {"in_chord": 1.0,
    "groove": 0.5, "empty_bars": -1.0}).  (windows (N, W, A) int64, mask (N, W) int64) on the GPU -> (N,) float32:
    r = sum over METRICS' order of weight * measure, each product and each sum rounded to float32 on its own (bitwise
    sampling.song_metrics_f32's reward).  One cwlt_song_metrics launch on the current stream with
    max_bars = min(W + 1, 512); no synchronisation; the output buffers are kept per shape, so a running loop allocates
    once (the returned tensor is overwritten by the next call of the same shape).

    A window is scored from its own rows alone: it starts at beat -1 with no chord, so a chord or a beat set before
    the window is not known to it, and notes in front of the window's first Beat row count for no beat and no chord.
    That is what makes a row's score independent of the rest of the pool.
    Refused: a name outside METRICS, a weight that is not finite (ValueError); CPU tensors (RuntimeError); W + 1 > 512
    (ValueError, at the first call)."""

    def __init__(self, word2event_or_spec, weights):
        self.spec = _as_spec(word2event_or_spec)
        table = np.zeros(len(METRICS), dtype=np.float32)
        for name, w in dict(weights).items():
            if name not in METRICS:
                raise ValueError("unknown metric %r (metrics: %s)" % (name, ", ".join(METRICS)))
            w = float(w)
            with np.errstate(over="ignore"):
                fits = np.isfinite(np.float32(w))
            if not np.isfinite(w) or not fits:
                raise ValueError("the weight of %r must be finite (in float32), got %r" % (name, w))
            table[METRICS.index(name)] = w
        self.weights = table
        self._buffers = {}

    def __call__(self, windows, mask=None):
        for t, name in ((windows, "windows"), (mask, "mask")):
            if t is not None and (not torch.is_tensor(t) or not t.is_cuda):
                raise RuntimeError("MetricReward: %s must be a GPU tensor: the cwlt hot path has no CPU implementation"
                                   % name)
        if windows.dim() != 3 or windows.shape[2] != len(self.spec.keys):
            raise ValueError("MetricReward: windows must be (N, W, %d), got %s" % (len(self.spec.keys),
                                                                                 tuple(windows.shape)))
        N, W, _ = windows.shape
        if W + 1 > MAX_BARS:
            raise ValueError("MetricReward: a window of %d rows may hold %d bar slots, at most %d are counted"
                             % (W, W + 1, MAX_BARS))
        key = (str(windows.device), N, W)
        buf = self._buffers.get(key)
        if buf is None:
            buf = (torch.empty(N, len(METRICS), dtype=torch.float32, device=windows.device),
                   torch.empty(N, dtype=torch.float32, device=windows.device),
                   torch.from_numpy(self.weights).to(windows.device))
            self._buffers[key] = buf
        feat, reward, weights = buf
        order, pitch, chord, table = self.spec.tables(windows.device, W + 1)
        ops.song_metrics(windows, mask, None, self.spec.attrs, order, pitch, chord, self.spec.Q, table,
                         min(W + 1, MAX_BARS), feat, weights=weights, reward=reward)
        return reward
