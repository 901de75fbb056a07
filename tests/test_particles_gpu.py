"""GPU: particle generation -- the three kernels of csrc/particles.hip one by one, then
generation.generate_particles end to end on the small fixture model (128 / 2 layers / 2 heads).

1. cwlt_particle_gather, bitwise against torch.index_select: rows 1, 2, 65, 300; rows of 8 B (the 8-byte path), 48 B
   (the 16-byte path), 339 floats (the 4-byte path, the fixture's logits width), 8192 floats x 3 blocks (the small
   model's S) with a block stride past the rows, and 48 B from a base one int off (4-byte path by alignment); ancestors
   the identity (sentinel-filled dst and scratch untouched), pairwise swaps through the two phases, all rows from one,
   random with repeats, one entry out of range (its row is left alone).  The repo-dims state, 32768 floats x 12 blocks,
   with 5 rows and with 30 rows: 30 x 12 x 8 work items are more than the launch's 2048 workgroups, so the grid-stride
   loop takes a second pass; the 4-byte path takes one at 300 rows x 3 blocks x 8192 floats from the odd base.
2. cwlt_particle_weigh, bitwise against sampling.particle_weigh_f32: rows 1 and 257, 6 and 8 attributes, a ring of 1 and
   of 5 rows with counters past the first wrap; done rows untouched; ending by the bar count and by the cap, on the row
   that reaches it.
3. cwlt_particle_resample against sampling.systematic_resample in float64, fed the kernel's own u: groups 1, 3, 130 x
   K 2, 7, 64, 65, 256, 1024 x the cases of tests/test_particles_cpu.py (equal, one dominant, 3 x normal, normal - 5000,
   done groups).  `resampled` agrees, ess to 1e-4 relative, ancestors are equal except where a threshold lies within
   (K + 2) 2^-23 s of a prefix-sum boundary -- the f32 error of expf plus any summation order -- and such entries are at
   most 1 % of the entries of each K (the CPU test shows that numpy float32 arithmetic on the same cases stays under
   it).  u in [0, 1), a function of (seed, event, group) alone.
4. End to end, 3 songs x 4 particles, bar_cond 4, max_tokens 48, resample_every 4: (i) - (v) of the tests below.
"""
import os

import numpy as np
import pytest
import torch

import rlmg_amd  # noqa: F401
from rlmg_amd import generation, ops, sampling
from rlmg_amd.generation import Constraint, Grammar, Preference

from test_blend_gpu import FIX, _bits, _same, _small_model, _word2event
from test_particles_cpu import CASES, GPU_GROUPS, GPU_KS, near_boundary, resample_case

pytestmark = pytest.mark.gpu
SENTINEL = -1234567
EPS = 2.0 ** -24


# ---- 1. gather -----------------------------------------------------------------------------------------------------------
def _ancestors(kind, rows, rng):
    n = np.arange(rows, dtype=np.int64)
    if kind == "identity":
        return n
    if kind == "swaps":
        a = n ^ 1
        a[a >= rows] = rows - 1                                         # an odd last row stays
        return a
    if kind == "from one":
        return np.full(rows, rows // 2, dtype=np.int64)
    a = rng.integers(0, rows, rows).astype(np.int64)
    if kind == "out of range":
        a[rng.integers(0, rows)] = rows if rows % 2 else -1
    return a


def _gather_case(cuda, rng, rows, row_ints, n_blocks, pad_ints, base_off, kinds):
    """One family of int32 buffers (n_blocks blocks of rows x row_ints, the blocks pad_ints further apart, the base
    base_off ints past an aligned address) through state -> scratch -> state for every kind of ancestor vector.  Whole
    buffers are compared: padding, the ints before the base and rows that do not move keep their values."""
    stride = rows * row_ints + pad_ints
    size = base_off + n_blocks * stride
    extent = (n_blocks - 1) * stride + rows * row_ints
    host = rng.integers(-2 ** 31, 2 ** 31, size, dtype=np.int64).astype(np.int32)

    def rows_of(t):                                                     # a (n_blocks, rows, row_ints) copy
        return t[base_off:].view(n_blocks, stride)[:, :rows * row_ints].reshape(n_blocks, rows, row_ints).clone()

    def with_rows(t, r):                                                # a copy of t with its rows replaced by r
        out = t.clone()
        out[base_off:].view(n_blocks, stride)[:, :rows * row_ints] = r.reshape(n_blocks, rows * row_ints)
        return out

    for kind in kinds:
        anc = _ancestors(kind, rows, rng)
        before = torch.as_tensor(host).to(cuda)
        state = before.clone()
        blank = torch.full_like(state, SENTINEL)
        scratch = blank.clone()
        anc_d = torch.as_tensor(anc).to(cuda)
        moved = (anc != np.arange(rows)) & (anc >= 0) & (anc < rows)
        mv = torch.as_tensor(np.nonzero(moved)[0]).to(cuda)
        args = (anc_d, 4 * row_ints, n_blocks, 4 * stride if n_blocks > 1 else 0)
        where = (kind, rows, row_ints, n_blocks, base_off)
        want_rows, scratch_rows = rows_of(before), rows_of(blank)
        if len(mv):
            want_rows[:, mv] = torch.index_select(rows_of(before), 1, anc_d[mv])
            scratch_rows[:, mv] = want_rows[:, mv]
        ops.particle_gather(scratch[base_off:base_off + extent], state[base_off:base_off + extent], *args)
        assert torch.equal(scratch, with_rows(blank, scratch_rows)), where + ("phase 1",)
        assert torch.equal(state, before), where                        # phase 1 only reads the state
        ops.particle_gather(state[base_off:base_off + extent], scratch[base_off:base_off + extent], *args,
                            copy_back=True)
        assert torch.equal(state, with_rows(before, want_rows)), where + ("phase 2",)
        assert torch.equal(scratch, with_rows(blank, scratch_rows)), where   # phase 2 only reads the scratch


KINDS = ("identity", "swaps", "from one", "random", "out of range")
LAYOUTS = {"8 B": (2, 1, 0, 0), "48 B": (12, 1, 0, 0), "339 floats": (339, 1, 0, 0),
           "8192 floats x 3": (8192, 3, 64, 0), "48 B, odd base": (12, 1, 0, 1)}


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_gather_against_index_select(cuda, layout):
    row_ints, n_blocks, pad, off = LAYOUTS[layout]
    rng = np.random.default_rng(list(LAYOUTS).index(layout))
    for rows in (1, 2, 65, 300):
        _gather_case(cuda, rng, rows, row_ints, n_blocks, pad, off, KINDS)


@pytest.mark.parametrize("rows,row_ints,n_blocks,off", [(5, 32768, 12, 0), (30, 32768, 12, 0), (300, 8192, 3, 1)])
def test_gather_past_one_grid(cuda, rows, row_ints, n_blocks, off):
    rng = np.random.default_rng(rows)
    _gather_case(cuda, rng, rows, row_ints, n_blocks, 0, off, ("random", "swaps"))


def test_gather_refusals(cuda):
    a = torch.zeros(64, dtype=torch.int32, device=cuda)
    b = torch.zeros(64, dtype=torch.int32, device=cuda)
    anc = torch.zeros(4, dtype=torch.int64, device=cuda)
    with pytest.raises(RuntimeError, match="1001"):
        ops.particle_gather(a, a, anc, 16)                              # in place
    with pytest.raises(ValueError, match="holds"):
        ops.particle_gather(a, b, anc, 128)                             # 4 rows x 128 B do not fit
    with pytest.raises(TypeError):
        ops.particle_gather(a, b, anc.to(torch.int32), 16)


# ---- 2. weigh ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("n_attr", [6, 8])
def test_weigh_against_f32_restatement(cuda, rows, n_attr):
    rng = np.random.default_rng(rows + n_attr)
    for out_rows, counters in ((1, (None, 3)), (5, (7, 13, 4))):
        for counter in counters:
            ring = (rng.normal(-3, 2, (out_rows, rows, n_attr, 2)) *
                    10.0 ** rng.integers(-3, 2, (out_rows, rows, n_attr, 2))).astype(np.float32)
            lw = rng.normal(0, 30, rows).astype(np.float32)
            length = rng.integers(0, 40, rows).astype(np.int64)
            bar = rng.integers(1, 4, rows).astype(np.int64)
            cap = length + rng.integers(2, 9, rows)
            done = (rng.random(rows) < 0.3).astype(np.int64) * rng.integers(1, 3, rows)
            bar_cond = 4
            # ends: row 0 reaches the bar count, the last row reaches its cap on this very row (when they are live)
            bar[0] = bar_cond
            cap[-1] = length[-1] + 1
            d = lambda x: torch.as_tensor(x).to(cuda)
            lw_d, len_d, done_d, ring_d = d(lw), d(length), d(done), d(ring)
            cnt = None if counter is None else torch.tensor([counter], dtype=torch.int64, device=cuda)
            ops.particle_weigh(ring_d, cnt, d(bar), bar_cond, d(cap), lw_d, len_d, done_d)
            o = 0 if counter is None else counter % out_rows
            live = done == 0
            want = sampling.particle_weigh_f32(lw, ring[o], done)
            got = lw_d.cpu().numpy()
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (rows, n_attr, out_rows, counter)
            assert np.array_equal(got[~live].view(np.int32), lw[~live].view(np.int32))
            assert np.array_equal(len_d.cpu().numpy(), length + live)
            ended = (bar >= bar_cond) | (length + 1 >= cap)
            assert np.array_equal(done_d.cpu().numpy(), np.where(live, ended.astype(np.int64), done))
            assert torch.equal(ring_d, d(ring))
            if live[0]:
                assert done_d[0].item() == 1                            # by the bar count
            if live[-1]:
                assert done_d[-1].item() == 1                           # by the cap, on the row that reaches it
            if rows > 2 and live[1] and bar[1] < bar_cond and length[1] + 1 < cap[1]:
                assert done_d[1].item() == 0


# ---- 3. resample ---------------------------------------------------------------------------------------------------------
def _resample(cuda, lw, done, K, ess_frac, seed, event, log_z0):
    groups = lw.shape[0]
    d = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(cuda)
    lw_d, lz = d(lw.reshape(-1)), d(log_z0)
    anc = torch.full((groups * K,), -7, dtype=torch.int64, device=cuda)
    u = torch.full((groups,), -1.0, dtype=torch.float32, device=cuda)
    ess = torch.full((groups,), -1.0, dtype=torch.float32, device=cuda)
    res = torch.full((groups,), -1, dtype=torch.int32, device=cuda)
    ops.particle_resample(lw_d, d(done.reshape(-1)), K, ess_frac, seed, event, anc, u, ess, res, lz)
    return (anc.cpu().numpy().reshape(groups, K), u.cpu().numpy(), ess.cpu().numpy(), res.cpu().numpy(),
            lz.cpu().numpy(), lw_d.cpu().numpy().reshape(groups, K))


@pytest.mark.parametrize("K", GPU_KS)
def test_resample_against_f64(cuda, K):
    entries = excused = 0
    for groups in GPU_GROUPS:
        for case in CASES:
            lw, done = resample_case(case, groups, K, seed=groups)
            rng = np.random.default_rng([K, groups, CASES.index(case)])
            log_z0 = rng.normal(0, 5, groups).astype(np.float32)
            anc, u, ess, res, log_z, lw_after = _resample(cuda, lw, done, K, 1.0, 99, 3, log_z0)
            assert ((u >= 0) & (u < 1)).all()
            for g in range(groups):
                want = sampling.systematic_resample(lw[g], u[g], 1.0, done=done[g])
                where = (case, groups, g)
                assert res[g] == want.resampled, where
                assert abs(ess[g] - want.ess) <= 1e-4 * want.ess, where
                own = anc[g] - g * K
                bad = own != want.anc
                if bad.any():
                    assert not (bad & ~near_boundary(want, K)).any(), where
                    excused += int(bad.sum())
                entries += K
                if want.resampled:
                    assert (lw_after[g] == 0).all(), where
                    x = lw[g].astype(np.float64)
                    m, inc = x.max(), want.log_z - x.max()
                    # f32: the sum s to (K + 2) 2^-23 relative (the bound above), logf and the two additions one
                    # rounding each of their results
                    bound = (K + 2) * 2.0 ** -23 + 4 * EPS * (abs(inc) + abs(want.log_z) + abs(log_z0[g] + want.log_z))
                    assert abs(float(log_z[g]) - (float(log_z0[g]) + want.log_z)) <= bound, (where, m)
                else:
                    assert np.array_equal(lw_after[g].view(np.int32), lw[g].view(np.int32)), where
                    assert log_z[g] == log_z0[g], where
            if case == "equal":
                assert not res.any() and (anc == np.arange(groups * K).reshape(groups, K)).all()
            if case == "dominant":
                assert res.all()
            if case == "done":
                assert not res[::2].any() and res[1::2].all()
    print("K = %d: %d of %d ancestors differ from float64, all within the excuse" % (K, excused, entries))
    assert excused <= 0.01 * entries


def test_resample_u_is_keyed_by_seed_event_group(cuda):
    K = 7
    lw130, done130 = resample_case("normal3", 130, K, seed=1)
    z = lambda g: np.zeros(g, dtype=np.float32)
    u130 = _resample(cuda, lw130, done130, K, 1.0, 5, 2, z(130))[1]
    again = _resample(cuda, lw130, done130, K, 1.0, 5, 2, z(130))[1]
    assert np.array_equal(u130, again)
    u3 = _resample(cuda, lw130[:3], done130[:3], K, 1.0, 5, 2, z(3))[1]
    assert np.array_equal(u3, u130[:3])                                 # group g's u: whatever the group count
    kept = _resample(cuda, lw130, done130, K, 0.0, 5, 2, z(130))
    assert np.array_equal(kept[1], u130) and not kept[3].any()         # and whatever the decision
    other_event = _resample(cuda, lw130, done130, K, 1.0, 5, 3, z(130))[1]
    other_seed = _resample(cuda, lw130, done130, K, 1.0, 6, 2, z(130))[1]
    assert (other_event != u130).mean() > 0.9 and (other_seed != u130).mean() > 0.9
    assert len(np.unique(u130)) > 120 and 0.3 < u130.mean() < 0.7


# ---- 4. end to end -------------------------------------------------------------------------------------------------------
N, K, BAR_COND, CAP, EVERY, SEED = 3, 4, 4, 48, 4, 21


@pytest.fixture(scope="module")
def world(cuda):
    seed = int(FIX["fill_seed"])
    w2e = _word2event()
    w = {"net": _small_model(cuda, seed), "ref": _small_model(cuda, seed + 1), "w2e": w2e}
    w["range"] = Constraint(w2e, allow={"tempo": ["tempo_3"], "pitch": range(5, 12)},
                            per_bar={"chord": [["chord_2"], ["chord_5", "chord_6"], [7]]}, cycle=True)
    w["tight"] = Constraint(w2e, per_bar={"pitch": [[5, 6, 7], [20, 21, 22], [40, 41, 42]]}, cycle=True)
    w["all on"] = dict(constraints=w["tight"], grammar=Grammar(w2e), reference=w["ref"], alpha=0.7,
                       preferences=Preference(w2e, repeat={"pitch": (0.5, 0.5)}, decay=0.9), sampler="categorical")
    return w


def _particles(w, n=N, **kw):
    torch.manual_seed(SEED)
    kw.setdefault("resample_every", EVERY)
    return generation.generate_particles(w["net"], w["w2e"], n, K, bar_cond=BAR_COND, max_tokens=CAP, chunk=16, **kw)


def _batch(w, n, **kw):
    torch.manual_seed(SEED)
    return generation.generate_batch(w["net"], w["w2e"], n, bar_cond=BAR_COND, max_tokens=CAP, chunk=16,
                                     return_logprobs=True, **kw)


def _flat(sets):
    return [s for ps in sets for s in ps.songs], [l for ps in sets for l in ps.logprobs]


def _same_sets(a, b):
    return (_same(a.songs, b.songs) and _bits(a.logprobs, b.logprobs) and
            np.array_equal(a.log_weights.view(np.int32), b.log_weights.view(np.int32)) and
            a.log_evidence == b.log_evidence and np.array_equal(a.ess.view(np.int32), b.ess.view(np.int32)) and
            np.array_equal(a.resampled, b.resampled) and np.array_equal(a.ancestors, b.ancestors) and
            np.array_equal(a.event_log_weights.view(np.int32), b.event_log_weights.view(np.int32)))


def test_ess_zero_is_generate_batch(world):
    """(i) ess = 0, with constraints: the songs and pairs of generate_batch(12, the lists repeated), bit for bit; the
    weights are the float32 sum of the returned pairs."""
    w = world
    cons = [w["range"], None, w["tight"]]
    sets = _particles(w, ess=0, constraints=cons)
    songs, lps = _batch(w, N * K, constraints=[c for c in cons for _ in range(K)])
    got, got_lp = _flat(sets)
    assert _same(got, songs) and _bits(got_lp, lps)
    assert len(sets) == N and all(len(ps.songs) == K for ps in sets)
    assert any(len(s) < CAP for s in songs)                             # some song ends by the bar rule
    for ps in sets:
        assert not ps.resampled.any() and (ps.ancestors == np.arange(K)).all()
        for k in range(K):
            lw = np.zeros(1, dtype=np.float32)
            for row in ps.logprobs[k]:
                lw = sampling.particle_weigh_f32(lw, row[None])
            assert lw.view(np.int32)[0] == ps.log_weights[k:k + 1].view(np.int32)[0]
        assert abs(ps.log_evidence - sampling.logmeanexp(ps.log_weights)) < 1e-12
        assert abs(ps.weights().sum() - 1) < 1e-12
    assert any(ps.log_weights.min() < -1 for ps in (sets[0], sets[2]))  # the constraints do cost mass
    assert len(sets[0].ess) >= 2


def test_unconstrained_categorical_never_resamples(world):
    """(ii) nothing is removed and nothing tempered: every weight is 0, no event resamples at the default ess, and the
    songs are generate_batch's."""
    w = world
    sets = _particles(w, sampler="categorical")
    songs, lps = _batch(w, N * K, sampler="categorical")
    got, got_lp = _flat(sets)
    assert _same(got, songs) and _bits(got_lp, lps)
    for ps in sets:
        assert len(ps.resampled) >= 2 and not ps.resampled.any() and (ps.log_weights == 0).all()
        assert (ps.ess == K).all() and ps.log_evidence == 0.0


def _host_ends(song, w2e, cap):
    """generate_batch's rule for a song from INIT_CW: it ends WITH the row that opens bar BAR_COND, or at cap rows."""
    cnt = 1
    for t in range(1, len(song)):
        cnt += w2e["bar-beat"][int(song[t, 2])] == "Bar"
        if cnt == BAR_COND:
            return t == len(song) - 1
    return len(song) == cap


def test_everything_on(world, monkeypatch):
    """(iii) a 3-pitch per-bar constraint, the grammar, a repetition penalty and a blend at alpha 0.7, ess = 1.

    The bounds.  log_weights[k] is a sequence of f32 operations on the pairs of the rows since the song's last
    resampling: n differences and n + n / 6 additions, each within 2^-24 of its result, results bounded by the sum of
    the |entries|: |lw - f64| <= (2 n + n / 6 + 1) 2^-24 sum |entries|.  log_evidence: per resampled event the kernel's
    increment from the recorded f32 weights -- the sum s to (K + 2) 2^-23 relative (expf to an ulp, K additions), logf
    and three additions to 2^-24 of their results -- and the final logmeanexp is formed in float64 from the same f32
    weights on both sides."""
    w = world
    kw = w["all on"]
    sets = _particles(w, ess=1.0, **kw)
    monkeypatch.setattr(ops, "GRAPHS_ENABLED", False)
    eager = _particles(w, ess=1.0, **kw)
    monkeypatch.undo()
    assert all(_same_sets(a, b) for a, b in zip(sets, eager))
    moved = sum(int((ps.ancestors != np.arange(K)).any(1).sum()) for ps in sets)
    print("everything on: %d events with a non-identity ancestor vector; lengths %s, log evidence %s"
          % (moved, [[len(s) for s in ps.songs] for ps in sets], [round(ps.log_evidence, 3) for ps in sets]))
    assert moved >= 1
    for ps in sets:
        assert (ps.ancestors[~ps.resampled] == np.arange(K)).all()
        assert (np.diff(ps.ancestors, axis=1) >= 0).all()
    songs, lps = _flat(sets)
    for s in songs:
        assert kw["constraints"].violations(s[1:], 1) == [] and kw["grammar"].violations(s, 1) == []
        assert _host_ends(s, w["w2e"], CAP), len(s)
    # a piece of state the gather does not carry breaks exactly this: the pairs are those of the song's own prefix
    score_kw = {k: v for k, v in kw.items()}
    scored = generation.score_songs(w["net"], w["w2e"], songs, **score_kw)
    worst = max(float(np.abs(lp - sc).max()) for lp, sc in zip(lps, scored))
    print("everything on: generated against scored log-probs, worst |difference| = %.3g" % worst)
    assert all(np.isfinite(lp).all() and lp.shape == (len(s) - 1, 6, 2) for s, lp in zip(songs, lps))
    assert worst <= 1e-4
    for ps in sets:
        E = len(ps.resampled)
        last = int(np.nonzero(ps.resampled)[0].max()) if ps.resampled.any() else -1
        for k in range(K):
            rows = ps.logprobs[k][(last + 1) * EVERY:].astype(np.float64)
            terms = rows[..., 0] - rows[..., 1]
            n = terms.size
            bound = (2 * n + n / 6 + 1) * EPS * np.abs(rows).sum()
            assert abs(float(ps.log_weights[k]) - terms.sum()) <= bound, (k, n)
        # the surviving lineages' weights at every event, from their own pairs
        line = generation.particle_lineage(ps.ancestors, K)
        for e in range(E):
            since = int(np.nonzero(ps.resampled[:e])[0].max()) + 1 if ps.resampled[:e].any() else 0
            for k in range(K):
                rows = ps.logprobs[k][since * EVERY:(e + 1) * EVERY].astype(np.float64)
                n = rows[..., 0].size
                bound = (2 * n + n / 6 + 1) * EPS * np.abs(rows).sum()
                seen = float(ps.event_log_weights[e, line[e, k]])
                assert abs(seen - (rows[..., 0] - rows[..., 1]).sum()) <= bound, (e, k)
        want, slack = 0.0, 0.0
        for e in np.nonzero(ps.resampled)[0]:
            x = ps.event_log_weights[e].astype(np.float64)
            inc = sampling.logmeanexp(x)
            want += inc
            slack += (K + 2) * 2.0 ** -23 + 4 * EPS * (abs(x.max()) + abs(inc - x.max()) + abs(inc) + abs(want))
        want += sampling.logmeanexp(ps.log_weights)
        assert abs(ps.log_evidence - want) <= slack + 1e-12, (ps.log_evidence, want, slack)
        assert np.isfinite(ps.log_evidence) and ps.log_evidence < 0


def test_song_zero_alone(world):
    """(iv) song 0's set does not depend on the other songs of the pool."""
    w = world
    kw = dict(w["all on"], ess=1.0)
    three = _particles(w, **kw)
    one = _particles(w, n=1, **kw)
    assert len(one) == 1 and _same_sets(one[0], three[0])
    assert three[0].resampled.any()


def test_refusals_and_generate(world, tmp_path):
    """(v)"""
    w = world
    net, w2e = w["net"], w["w2e"]
    for kw, msg in ((dict(particles=1), "particles must be"), (dict(particles=1025), "particles must be"),
                    (dict(n_songs=1025, particles=4), "at most 4096"), (dict(resample_every=0), "resample_every"),
                    (dict(ess=1.01), "ess must"), (dict(sampler="greedy"), "sampler must"),
                    (dict(reference=w["ref"]), "needs alpha="), (dict(prefill="fast"), "must be 'blas' or 'gemm'"),
                    (dict(max_tokens=1), "leaves no room"), (dict(constraints=[None, None]), "constraints")):
        args = dict(n_songs=3, particles=4)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            generation.generate_particles(net, w2e, **args)
    net.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            generation.generate_particles(net, w2e, 3, 4)
    finally:
        net.eval()
    with pytest.raises(ValueError, match="pass batch_size"):
        generation.generate(net, w2e, n_songs=3, particles=4, path_gendir=str(tmp_path))
    kw = dict(constraints=w["tight"], grammar=w["all on"]["grammar"], ess=1.0, resample_every=EVERY)
    torch.manual_seed(SEED)
    sets = generation.generate_particles(net, w2e, 3, 4, bar_cond=BAR_COND, max_tokens=CAP, **kw)
    torch.manual_seed(SEED)
    stats = generation.generate(net, w2e, n_songs=3, bar_cond=BAR_COND, max_tokens=CAP, batch_size=3, particles=4,
                                path_gendir=str(tmp_path), stats_path=str(tmp_path / "stats.json"), log=lambda s: None,
                                logprobs=True, **kw)
    assert len(stats["words_len_list"]) == 3
    for i, ps in enumerate(sets):
        song = np.load(os.path.join(str(tmp_path), "get_%d.npy" % i))
        lp = np.load(os.path.join(str(tmp_path), "get_%d_logp.npy" % i))
        hits = [k for k in range(4) if song.shape == ps.songs[k].shape and (song == ps.songs[k]).all()]
        assert hits and len(song) == stats["words_len_list"][i]
        assert any(np.array_equal(lp.view(np.int32), ps.logprobs[k].view(np.int32)) for k in hits)
    # particles=None changes nothing
    torch.manual_seed(SEED)
    a = generation.generate(net, w2e, n_songs=3, bar_cond=BAR_COND, max_tokens=CAP, batch_size=3,
                            path_gendir=str(tmp_path / "a"), stats_path=None, log=lambda s: None)
    torch.manual_seed(SEED)
    b = generation.generate_batch(net, w2e, 3, bar_cond=BAR_COND, max_tokens=CAP)
    assert a["words_len_list"] == [len(s) for s in b]
