"""Dataset plumbing for the entry scripts: the reference's on-disk formats when the files exist, synthetic
data of the same schema otherwise (the dataset and the pretrained weights are external downloads,
README.md:23,27 -- unavailable offline).

  dqn: train_data_linear.npz {x, y (N, 3584, 7) int, mask (N, 3584)} + dictionary.pkl = (event2word, word2event)
       keyed tempo, chord, bar-beat, type, pitch, duration, velocity      (IRL_dqn_train.py:389-391,418-420)
  ppo: dictionary.pickle + our_dataset.pickle {train_x, train_y (N, 1200, 6), mask (N, 1200)}
       (ppo_train.py:432-449, preprocess.py:66-72)
"""
import os
import pickle

import numpy as np

DQN_KEYS = ("tempo", "chord", "bar-beat", "type", "pitch", "duration", "velocity")
DQN_N = (56, 135, 18, 3, 87, 18, 25)             # IRL_dqn_train.py:403 (+ 3 `type` classes)
PPO_KEYS = ("Tempo", "Bar", "Position", "Pitch", "Duration", "Velocity")
PPO_N = (49, 19, 19, 89, 67, 25)                 # prepare_data.py:247-291


def _synth(n_seq, T, n_per_field, seed):
    rng = np.random.default_rng(seed)
    x = np.stack([rng.integers(0, n, (n_seq, T)) for n in n_per_field], -1).astype(np.int64)
    y = np.stack([rng.integers(0, n, (n_seq, T)) for n in n_per_field], -1).astype(np.int64)
    mask = np.ones((n_seq, T), dtype=np.float32)
    mask[: n_seq // 2, int(T * 0.9):] = 0
    return x, y, mask


def synthetic_cp_vocabulary():
    """word2event of the same shape as the compound-word dictionary the reference trains on (class counts of
    IRL_dqn_train.py:403; event spellings as dqn_policy/testing-no-type-cp.py:56-117 parses them: 0 = ignore,
    'CONTI', 'Bar', 'Beat_<k>', 'Tempo_<bpm>', 'Note_Pitch_<p>', 'Note_Duration_<ticks>', 'Note_Velocity_<v>')."""
    tempo = [0, "CONTI"] + ["Tempo_%d" % (32 + 3 * i) for i in range(DQN_N[0] - 2)]
    roots = ["C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"]
    quals = ["M", "m", "o", "+", "7", "M7", "m7", "o7", "/o7", "sus2", "sus4"]
    chord = ([0, "CONTI"] + ["%s_%s" % (r, q) for r in roots for q in quals] + ["N_N"])[:DQN_N[1]]
    barbeat = [0, "Bar"] + ["Beat_%d" % i for i in range(DQN_N[2] - 2)]
    typ = ["EOS", "Metrical", "Note"]
    pitch = [0] + ["Note_Pitch_%d" % (22 + i) for i in range(DQN_N[4] - 1)]
    duration = [0] + ["Note_Duration_%d" % (120 * (i + 1)) for i in range(DQN_N[5] - 1)]
    velocity = [0] + ["Note_Velocity_%d" % (40 + 2 * i) for i in range(DQN_N[6] - 1)]
    cols = (tempo, chord, barbeat, typ, pitch, duration, velocity)
    assert tuple(len(c) for c in cols) == DQN_N
    return {k: dict(enumerate(c)) for k, c in zip(DQN_KEYS, cols)}


def load_dqn(path_train_data, path_dictionary, n_seq=8, T=3584, seed=1234):
    """-> (event2word, word2event), {x, y, mask}; synthetic when the files are absent."""
    if os.path.exists(path_train_data) and os.path.exists(path_dictionary):
        with open(path_dictionary, "rb") as f:
            dictionary = pickle.load(f)
        d = np.load(path_train_data)
        return dictionary, {"x": d["x"], "y": d["y"], "mask": d["mask"]}
    print("[data] %s not found: using synthetic CW tokens of the same schema" % path_train_data)
    w2e = synthetic_cp_vocabulary()
    e2w = {k: {e: i for i, e in v.items()} for k, v in w2e.items()}
    x, y, mask = _synth(n_seq, T, DQN_N, seed)
    return (e2w, w2e), {"x": x, "y": y, "mask": mask}


def ppo_vocabulary():
    """event2word of the PPO pipeline.  Unlike the CP dictionary it does not depend on the dataset: it is the fixed
    table ppo_policy/prepare_data.py:240-296 builds (value ranges per event type + <BOS>/<EOS>/<PAD>), so the
    synthetic stand-in is the real vocabulary."""
    values = {"Tempo": ["%d" % i for i in range(28, 211, 4)], "Bar": ["%d" % i for i in range(16)],
              "Position": ["%d/16" % i for i in range(16)], "Pitch": ["%d" % i for i in range(22, 108)],
              "Duration": ["%d" % i for i in range(64)], "Velocity": ["%d" % i for i in range(22)]}
    e2w = {}
    for k in PPO_KEYS:
        names = ["%s %s" % (k, v) for v in values[k]] + ["%s <BOS>" % k, "%s <EOS>" % k, "%s <PAD>" % k]
        e2w[k] = {name: i for i, name in enumerate(names)}
    assert tuple(len(e2w[k]) for k in PPO_KEYS) == PPO_N
    return e2w


def load_ppo(path_dictionary, path_train_data, n_seq=8, T=1200, seed=1234):
    if os.path.exists(path_train_data) and os.path.exists(path_dictionary):
        with open(path_dictionary, "rb") as f:
            dictionary = pickle.load(f)
        with open(path_train_data, "rb") as f:
            ds = pickle.load(f)
        return dictionary, ds
    print("[data] %s not found: using synthetic CW tokens of the same schema" % path_train_data)
    e2w = ppo_vocabulary()
    w2e = {k: {i: e for e, i in v.items()} for k, v in e2w.items()}
    x, y, mask = _synth(n_seq, T, PPO_N, seed)
    return (e2w, w2e), {"train_x": x, "train_y": y, "mask": mask}


# ----------------------------------------------------------------------------------------------------------------------
# packed variable-length batches: songs laid end to end in one row buffer (CWTrunk.train_step_packed)
# ----------------------------------------------------------------------------------------------------------------------
class PackedBatch:
    """Songs of different lengths end to end.  tokens, target (R, A) int64, mask (R) f32, pos (R) int32 (the position of
    a row inside its song), cu (n_songs + 1) int32 row offsets -- all on `device` -- with cu_host, the same offsets as a
    tuple of ints, and songs, the dataset indices in packed order (-1: the filler song of pad_rows_to)."""

    def __init__(self, tokens, target, mask, cu, cu_host, pos, songs):
        self.tokens, self.target, self.mask, self.cu, self.cu_host, self.pos, self.songs = (tokens, target, mask, cu,
                                                                                            cu_host, pos, songs)

    @property
    def rows(self):
        return self.cu_host[-1]

    @property
    def max_len(self):
        return max(b - a for a, b in zip(self.cu_host, self.cu_host[1:]))


def song_lengths(mask):
    """(N, T) loss mask -> (N) int64: a song's length is its last live row plus 1 (0: no live row at all)."""
    m = np.asarray(mask) != 0
    T = m.shape[1]
    return np.where(m.any(1), T - np.argmax(m[:, ::-1], axis=1), 0).astype(np.int64)


def pack_songs(x, y, mask, indices, pad_rows_to=None, device=None, lengths=None):
    """The songs `indices` of x, y (N, T, A), mask (N, T) as one PackedBatch, longest first (ties in the order given) so
    the scan launch's tail is short.  Rows past a song's last live mask row are dropped; holes inside it stay, with their
    mask 0.  pad_rows_to = k: one filler song (tokens 0, mask 0) is appended so that R % k == 0.  A song with no live
    row is refused: the scan has no empty streams."""
    import torch
    indices = [int(i) for i in indices]
    if not indices:
        raise ValueError("pack_songs needs at least one song")
    if lengths is None:
        lengths = song_lengths(np.asarray(mask)[indices])
    else:
        lengths = np.asarray(lengths, dtype=np.int64)[indices]
    if (lengths <= 0).any():
        raise ValueError("song %d has no live mask row: an empty song cannot be packed"
                         % indices[int(np.argmax(lengths <= 0))])
    order = np.argsort(-lengths, kind="stable")
    songs = [indices[i] for i in order]
    lens = [int(lengths[i]) for i in order]
    A = x.shape[2]
    R = sum(lens)
    fill = (-R) % int(pad_rows_to) if pad_rows_to else 0
    tok = np.zeros((R + fill, A), dtype=np.int64)
    tgt = np.zeros((R + fill, A), dtype=np.int64)
    msk = np.zeros(R + fill, dtype=np.float32)
    pos = np.zeros(R + fill, dtype=np.int32)
    cu = [0]
    for s, n in zip(songs, lens):
        a = cu[-1]
        tok[a:a + n], tgt[a:a + n], msk[a:a + n] = x[s, :n], y[s, :n], mask[s, :n]
        pos[a:a + n] = np.arange(n)
        cu.append(a + n)
    if fill:
        pos[R:] = np.arange(fill)
        cu.append(R + fill)
        songs = songs + [-1]
    if device is None:
        device = "cuda"
    t = lambda a: torch.from_numpy(a).to(device)
    return PackedBatch(t(tok), t(tgt), t(msk), torch.tensor(cu, dtype=torch.int32, device=device), tuple(cu), t(pos),
                       songs)


def _packed_groups(all_len, indices, rows_per_step, seed, max_len):
    """The epoch's batches as lists of song indices: `indices` in the order of a permutation drawn from `seed`, cut
    greedily (a batch closes when the next song does not fit).  Host arithmetic on the lengths only."""
    for i in indices:
        n = int(all_len[i])
        if n <= 0:
            raise ValueError("song %d has no live mask row: an empty song cannot be packed" % i)
        if n > rows_per_step:
            raise ValueError("song %d has %d rows, more than rows_per_step = %d" % (i, n, rows_per_step))
        if max_len is not None and n > max_len:
            raise ValueError("song %d has %d rows, more than the positional table (%d)" % (i, n, max_len))
    groups, cur, rows = [], [], 0
    for j in np.random.default_rng(seed).permutation(len(indices)):
        i = indices[j]
        n = int(all_len[i])
        if cur and rows + n > rows_per_step:
            groups.append(cur)
            cur, rows = [], 0
        cur.append(i)
        rows += n
    if cur:
        groups.append(cur)
    return groups


def packed_groups(mask, rows_per_step, seed, max_len=None, indices=None, rank=0, world=1):
    """The song indices of every batch packed_batches yields for the same arguments (a list of lists), from the lengths
    alone: nothing is packed or uploaded.  len() of it is the epoch's step count."""
    rows_per_step = int(rows_per_step)
    indices = list(range(len(mask))) if indices is None else [int(i) for i in indices]
    all_len = song_lengths(mask)
    per_rank = [_packed_groups(all_len, indices[r::world], rows_per_step, seed, max_len) for r in range(world)]
    return per_rank[rank][:min(len(g) for g in per_rank)]


def packed_batches(x, y, mask, rows_per_step, seed, max_len=None, indices=None, pad_rows_to=None, device=None,
                   rank=0, world=1):
    """One epoch of PackedBatches of at most rows_per_step rows (filler included): the songs (`indices`, default all) in
    the order of a permutation drawn from `seed`, cut greedily -- a batch closes when the next song does not fit -- so
    every song appears exactly once and the same seed gives the same batches.  max_len: the positional table's length.
    A song longer than rows_per_step or max_len is refused before anything is yielded.
    world > 1 (data parallelism): rank r packs its own stride indices[r::world]; every rank yields the batch count of
    the rank with the fewest (each works it out from the lengths alone), so that the ranks take the same number of
    steps -- the songs of the surplus batches sit out that epoch."""
    if pad_rows_to and int(rows_per_step) % int(pad_rows_to):
        raise ValueError("rows_per_step must be a multiple of pad_rows_to")
    groups = packed_groups(mask, rows_per_step, seed, max_len, indices, rank, world)
    all_len = song_lengths(mask)
    return (pack_songs(x, y, mask, g, pad_rows_to, device, lengths=all_len) for g in groups)      # one batch at a time
