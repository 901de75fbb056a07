"""GPU: the packed form of the causal linear attention scans (songs of different lengths end to end in one row buffer,
cwlt_causal_linear_*_packed) on all four routes of tests/test_cla_f64_gpu.py: f32, generic, mfma, sweep.

Exact equality is the check on the offsets: for every song, the packed run's out, zinv, dq, dk, dv rows, final state and
per-stream column sums are BITWISE those of the rectangular entry point run on that song alone (N = 1, L = its length,
the same route, CWLT_SCAN_SEGMENTS=1) -- the packed kernels are the same kernels instantiated with a row-offset table, and
a song's chunking starts at its own row 0.  The accuracy the existing f64 tests established is inherited through it.

Standing on its own, the first length set is also held row by row to oracle.cla_f64.reference under
oracle.cla_f64.bounds(form, ...) unchanged, with the vacuous-row cap of 2 % of tests/test_cla_f64_gpu.py: the worst
tensor's share, its rows pooled over the songs of the set (a share per song means nothing for songs of 1 and 2 rows;
tests/test_packed_cpu.py asserts on the CPU that the reference alone stays within that cap).

Isolation: rows after row R of every buffer and the padding columns of the strided (generic) case are NaN and are neither
read nor written; replacing one song's inputs leaves every other song's outputs bitwise unchanged; a second run repeats
bitwise.  The summed dbias is held to oracle.cla_f64.colsum_bound as check_colsum does there.

Length sets: 9 songs (plain stream order) at H = 2; 8 songs, deliberately unsorted (XCD-dealt order) at H = 3 and 8; 16
songs at H = 1.  Lengths 1, 2, one short of / exactly / one past one, two and four chunks of 64, ragged middles.
"""
import pytest
import torch

import rlmg_amd  # noqa: F401
from rlmg_amd import _lib, ops
from oracle import cla_f64 as o

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
NAMES = ("out", "dq", "dk", "dv")
ROUTES = ["f32", "generic", "mfma", "sweep"]
SET_A = [1, 2, 63, 64, 65, 127, 128, 129, 200]
SET_B = [130, 1, 64, 257, 65, 3, 192, 128]
SET_C = [1, 2, 63, 64, 65, 127, 128, 129, 200, 130, 3, 257, 192, 64, 65, 1]
CASES = [("A", SET_A, 2), ("B", SET_B, 3), ("B", SET_B, 8), ("C", SET_C, 1)]
TAIL = 5          # NaN rows after row R of every buffer
REAL_CALL = ops._call
_CACHE = {}


def song_inputs(lens, H, dtype, cuda):
    """Per song q, k, v, dout (1, L, H, 64) on the GPU, drawn separately (seed = song number): shared, never modified."""
    key = (tuple(lens), H, dtype)
    if key not in _CACHE:
        _CACHE[key] = [tuple(t.to(cuda) for t in o.make_inputs("randn", 1, L, H, 100 + s, dtype))
                       for s, L in enumerate(lens)]
    return _CACHE[key]


def offsets(lens, cuda):
    cu = [0]
    for L in lens:
        cu.append(cu[-1] + L)
    return ops.SeqOffsets(cu, device=cuda)


def packed_buffers(songs, route):
    """q, k, v as (R, H, 64) views of one NaN-filled (R + TAIL, 3 H 64 + pad) buffer (pad = 4 columns on the generic
    route, so the row stride is no multiple of 8), dout a view of a NaN-tailed buffer of its own."""
    H = songs[0][0].shape[2]
    R = sum(s[0].shape[1] for s in songs)
    dtype, dev = songs[0][0].dtype, songs[0][0].device
    W = 3 * H * 64 + (4 if route == "generic" else 0)
    buf = torch.full((R + TAIL, W), float("nan"), dtype=dtype, device=dev)
    views = []
    for i in range(3):
        view = buf.as_strided((R, H, 64), (W, 64, 1), i * H * 64)
        view.copy_(torch.cat([s[i][0] for s in songs], 0))
        views.append(view)
    gbuf = torch.full((R + TAIL, H, 64), float("nan"), dtype=dtype, device=dev)
    gbuf[:R] = torch.cat([s[3][0] for s in songs], 0)
    return buf, views, gbuf, gbuf[:R]


@pytest.fixture
def calls(monkeypatch):
    log = []

    def spy(name, *args, **kw):
        if name.startswith("cwlt_causal_linear"):
            log.append(name[len("cwlt_causal_linear_"):])
        return REAL_CALL(name, *args, **kw)

    monkeypatch.setattr(ops, "_call", spy)
    monkeypatch.setenv("CWLT_SCAN_SEGMENTS", "1")
    return log


PACKED_CALLS = {"f32": ["fwd_packed", "bwd_dkdv_packed", "bwd_dq_packed"],
                "generic": ["fwd_packed", "bwd_dkdv_packed", "bwd_dq_packed"],
                "mfma": ["fwd_packed", "bwd_dkdv_packed", "bwd_dq_packed"], "sweep": ["fwd_packed", "bwd_sweep_packed"]}


def run_packed(route, songs, cu, log, per_song=True):
    """The packed run through the package's wrappers -> dict of out, zinv, dq, dk, dv (R, ...), [cs (3, S, H 64), dbias,
    fin (S, H, 65 * 64)], plus the input buffers for the NaN checks."""
    buf, (q, k, v), gbuf, g = packed_buffers(songs, route)
    fast = route in ("mfma", "sweep")
    del log[:]
    res = {}
    if route == "sweep":
        q2, k2, v2, out, zinv, fin = ops.cla_fwd_packed(q, k, v, cu, final_state=True)
        assert fin is not None
        res["fin"] = fin.view(cu.n_songs, -1, 65 * 64)
    else:
        q2, k2, v2, out, zinv = ops.cla_fwd_packed(q, k, v, cu)
        fin = None
    assert q2.data_ptr() == q.data_ptr(), "the strided views are taken as they are"
    back = ops.cla_bwd_packed(q2, k2, v2, out, zinv, g, cu, want_colsum=fast, final_state=fin, per_song=fast)
    torch.cuda.synchronize()
    assert log == PACKED_CALLS[route], log
    dqkv = back[0] if fast else back
    if fast:
        res["cs"] = back[1]
        res["dbias"] = back[1].sum(1).reshape(-1)
    res.update(out=out, zinv=zinv, dq=dqkv[:, 0], dk=dqkv[:, 1], dv=dqkv[:, 2], buf=buf, gbuf=gbuf)
    return res


def run_alone(route, song, log):
    """One song through the existing rectangular entry points on the same route."""
    q, k, v, g = song
    del log[:]
    if route == "generic":
        N, L, H, _ = q.shape
        W = 3 * H * 64 + 4
        buf = torch.full((N, L, W), float("nan"), dtype=q.dtype, device=q.device)
        views = []
        for i, t in enumerate((q, k, v)):
            view = buf.as_strided((N, L, H, 64), (L * W, W, 64, 1), i * H * 64)
            view.copy_(t)
            views.append(view)
        q, k, v = views
    res = {}
    fast = route in ("mfma", "sweep")
    if route == "sweep":
        q, k, v, out, zinv, fin = ops.cla_fwd(q, k, v, final_state=True)
        assert fin is not None
        res["fin"] = fin
    else:
        q, k, v, out, zinv = ops.cla_fwd(q, k, v)
        fin = None
    back = ops.cla_bwd(q, k, v, out, zinv, g, want_colsum=fast, final_state=fin)
    torch.cuda.synchronize()
    assert log == [n.replace("_packed", "") for n in PACKED_CALLS[route]], log
    dqkv = back[0] if fast else back
    if fast:
        res["cs"] = back[1]
    res.update(out=out[0], zinv=zinv[0], dq=dqkv[0, :, 0], dk=dqkv[0, :, 1], dv=dqkv[0, :, 2])
    return res


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("name,lens,H", CASES)
@pytest.mark.parametrize("route", ROUTES)
def test_every_song_is_bitwise_the_song_alone(cuda, calls, route, name, lens, H):
    dtype = F32 if route == "f32" else BF16
    songs = song_inputs(lens, H, dtype, cuda)
    cu = offsets(lens, cuda)
    res = run_packed(route, songs, cu, calls)
    for s, L in enumerate(lens):
        a, z = cu.host[s], cu.host[s + 1]
        alone = run_alone(route, songs[s], calls)
        for n in NAMES + ("zinv",):
            assert same_bits(res[n][a:z], alone[n]), (route, name, H, "song %d (L = %d)" % (s, L), n)
        if route == "sweep":
            assert same_bits(res["fin"][s].reshape(-1), alone["fin"]), (route, name, H, s, "final state")
        if "cs" in res:
            assert same_bits(res["cs"][:, s].reshape(-1), alone["cs"]), (route, name, H, s, "column sums")
    # rows after R and the padding columns: not read (every output is finite) and not written (still NaN)
    for n in NAMES + ("zinv",):
        assert torch.isfinite(res[n].float()).all(), (route, n)
    R = cu.rows
    assert torch.isnan(res["buf"][R:].float()).all() and torch.isnan(res["gbuf"][R:].float()).all()
    if route == "generic":
        assert torch.isnan(res["buf"][:, 3 * H * 64:].float()).all()


@pytest.mark.parametrize("route", ROUTES)
def test_first_set_rows_against_f64(cuda, calls, route):
    """Every row of every song of the first set against the f64 reference of that song, bounds(form, ...) unchanged."""
    lens, H = SET_A, 2
    dtype = F32 if route == "f32" else BF16
    songs = song_inputs(lens, H, dtype, cuda)
    cu = offsets(lens, cuda)
    res = run_packed(route, songs, cu, calls)
    worst = {n: 0.0 for n in NAMES + ("zinv",)}
    loose_rows, rows = {n: 0 for n in NAMES}, {n: 0 for n in NAMES}
    for s, L in enumerate(lens):
        a, z = cu.host[s], cu.host[s + 1]
        ref = o.reference(*songs[s], kf_round=o.rb)
        t = o.analyse(ref)
        b = o.bounds(route, ref, t, L)
        for n in NAMES:
            r = o.row_ratio(res[n][a:z].unsqueeze(0), ref[n], t["den_" + n]) / b[n]
            loose = b[n] > 1
            worst[n] = max(worst[n], torch.where(loose, torch.zeros_like(r), r).max().item())
            if n in ("dq", "dk"):
                loose = loose[:, 1:]
            loose_rows[n] += int(loose.sum().item())
            rows[n] += loose.numel()
        zr = (res["zinv"][a:z].unsqueeze(0).double() - ref["zinv"]).abs() / ref["zinv"]
        kap = 4 * 2 ** 0.5 * o.phi_abs_term(ref) if route in ("f32", "generic") else 0.0
        worst["zinv"] = max(worst["zinv"], (zr / (o.zinv_bound(route, L) ** 2 + kap ** 2) ** 0.5).max().item())
    vacuous = max(loose_rows[n] / rows[n] for n in NAMES)     # the worst tensor, its rows pooled over the songs
    print("    packed %-8s %s  vacuous %.4f" % (route, "  ".join("%s %.2f" % kv for kv in worst.items()), vacuous))
    assert max(worst.values()) <= 1.0, (route, worst)
    assert vacuous <= 0.02, (route, "rows whose bound is above 1", loose_rows, rows)


@pytest.mark.parametrize("route", ["mfma", "sweep"])
def test_summed_dbias(cuda, calls, route):
    """dbias (3 H 64) against the f64 sums of the stored gradients over the R packed rows (check_colsum's measure)."""
    lens, H = SET_B, 3
    songs = song_inputs(lens, H, BF16, cuda)
    cu = offsets(lens, cuda)
    buf, (q, k, v), gbuf, g = packed_buffers(songs, route)
    q, k, v, out, zinv, fin = ops.cla_fwd_packed(q, k, v, cu, final_state=route == "sweep")
    dqkv, dbias = ops.cla_bwd_packed(q, k, v, out, zinv, g, cu, want_colsum=True, final_state=fin)
    assert dbias.shape == (3 * H * 64,)
    worst = 0.0
    for i, n in enumerate(("dq", "dk", "dv")):
        x = dqkv[:, i].double()
        want, sabs, rss = x.sum(0).reshape(-1), x.abs().sum(0).reshape(-1), (x ** 2).sum(0).sqrt().reshape(-1)
        allow = o.colsum_bound(cu.rows) * sabs + (4 * 2 * o.U16 * rss if route == "mfma" and n != "dv" else 0)
        got = dbias.double().reshape(3, -1)[i]
        worst = max(worst, ((got - want).abs() / allow.clamp_min(1e-300)).max().item())
    print("    packed %s column sums %.2f" % (route, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("route", ROUTES)
def test_songs_do_not_see_each_other_and_runs_repeat(cuda, calls, route):
    lens, H = SET_B, 3
    dtype = F32 if route == "f32" else BF16
    songs = song_inputs(lens, H, dtype, cuda)
    cu = offsets(lens, cuda)
    first = run_packed(route, songs, cu, calls)
    again = run_packed(route, songs, cu, calls)
    for n in NAMES + ("zinv",) + (("cs",) if "cs" in first else ()) + (("fin",) if "fin" in first else ()):
        assert same_bits(first[n], again[n]), (route, n, "a second run repeats bitwise")
    j = 3                                                     # the longest song, in the middle of the buffer
    other = list(songs)
    other[j] = tuple(t.to(cuda) for t in o.make_inputs("x3", 1, lens[j], H, 999, dtype))
    res = run_packed(route, other, cu, calls)
    a, z = cu.host[j], cu.host[j + 1]
    for n in NAMES + ("zinv",):
        assert same_bits(res[n][:a], first[n][:a]) and same_bits(res[n][z:], first[n][z:]), (route, n)
        assert not same_bits(res[n][a:z], first[n][a:z]), (route, n, "the replaced song itself changes")
    for n in ("cs", "fin"):
        if n in first:
            keep = [s for s in range(len(lens)) if s != j]
            x, y = (first[n], res[n]) if n == "fin" else (first[n].transpose(0, 1), res[n].transpose(0, 1))
            assert same_bits(x[keep], y[keep]), (route, n)


@pytest.mark.parametrize("route", ROUTES)
def test_outputs_past_the_end_and_padding_columns_are_not_written(cuda, calls, route):
    """The write side of the isolation: the C entry points called directly with OUTPUT buffers of R + TAIL rows (and, on
    the generic route, 4 padding columns per row of out and of dq | dk | dv) filled with NaN beforehand, and per-stream
    buffers (final state, column sums) with one stream to spare.  Everything past row R, every padding column and the
    spare stream are still NaN afterwards; what was written is bitwise the wrappers' result."""
    lens, H = SET_B, 3
    dtype = F32 if route == "f32" else BF16
    songs = song_inputs(lens, H, dtype, cuda)
    cu = offsets(lens, cuda)
    want = run_packed(route, songs, cu, calls)
    R, S, HD = cu.rows, cu.n_songs, H * 64
    pad = 4 if route == "generic" else 0
    fast = route in ("mfma", "sweep")
    nan = lambda shape, dt: torch.full(shape, float("nan"), dtype=dt, device=cuda)
    buf, (q, k, v), gbuf, g = packed_buffers(songs, route)
    ob, zb, db = nan((R + TAIL, HD + pad), dtype), nan((R + TAIL, H), F32), nan((R + TAIL, 3 * HD + pad), dtype)
    ddb, finb, csb = nan((R + TAIL, H), F32), nan((S + 1, H * 65 * 64), F32), nan((3, S + 1, HD), F32)
    esz = ob.element_size()
    ptr = lambda t, off=0: _lib.ctypes.c_void_p(t.data_ptr() + off * esz)
    ldi, ldo, ldd = q.stride(0), HD + pad, 3 * HD + pad
    code, st = _lib.dtype_code(dtype), _lib.stream_ptr()
    head = (ptr(cu.dev), S, H, 64)
    common = (ptr(q), ptr(k), ptr(v), ptr(ob), ptr(zb), ptr(g))
    cs = [ptr(csb[i]) if fast else None for i in range(3)]
    REAL_CALL("cwlt_causal_linear_fwd_packed", ptr(q), ptr(k), ptr(v), ptr(ob), ptr(zb), *head, ldi, ldi, ldi, ldo, 1e-6,
              ptr(finb) if route == "sweep" else None, code, st)
    if route == "sweep":
        REAL_CALL("cwlt_causal_linear_bwd_sweep_packed", *common, ptr(finb), ptr(db), ptr(db, HD), ptr(db, 2 * HD), *cs,
                  *head, ldi, ldi, ldi, ldo, HD, ldd, ldd, ldd, code, st)
    else:
        dden = ptr(ddb) if fast else None
        REAL_CALL("cwlt_causal_linear_bwd_dkdv_packed", *common, ptr(db, HD), ptr(db, 2 * HD), cs[1], cs[2], dden, *head,
                  ldi, ldi, ldi, ldo, HD, ldd, ldd, code, st)
        REAL_CALL("cwlt_causal_linear_bwd_dq_packed", *common, ptr(db), cs[0], dden, *head, ldi, ldi, ldi, ldo, HD, ldd,
                  code, st)
    torch.cuda.synchronize()
    isnan = lambda t: bool(torch.isnan(t.float()).all())
    assert isnan(ob[R:]) and isnan(zb[R:]) and isnan(db[R:]), (route, "rows past R were written")
    if pad:
        assert isnan(ob[:, HD:]) and isnan(db[:, 3 * HD:]), (route, "padding columns were written")
    assert same_bits(ob[:R, :HD].reshape(R, H, 64), want["out"]) and same_bits(zb[:R], want["zinv"])
    for i, n in enumerate(("dq", "dk", "dv")):
        assert same_bits(db[:R, i * HD:(i + 1) * HD].reshape(R, H, 64), want[n]), (route, n)
    if fast:
        assert isnan(csb[:, S]) and same_bits(csb[:, :S], want["cs"]), (route, "column sums")
    if route == "mfma":
        assert isnan(ddb[R:]) and bool(torch.isfinite(ddb[:R]).all()), (route, "dden")
    if route == "sweep":
        assert isnan(finb[S]) and same_bits(finb[:S].view(S, H, 65 * 64), want["fin"]), (route, "final state")


def test_wrapper_refusals(cuda):
    H = 2
    q = torch.zeros(10, H, 64, dtype=BF16, device=cuda)
    with pytest.raises(ValueError, match="strictly increasing"):
        ops.cla_fwd_packed(q, q, q, [0, 4, 4, 10])
    with pytest.raises(ValueError, match="strictly increasing"):
        ops.cla_fwd_packed(q, q, q, [0, 6, 4, 10])
    with pytest.raises(ValueError, match="ends at row"):
        ops.cla_fwd_packed(q, q, q, [0, 4, 9])
    with pytest.raises(ValueError, match="starting at 0"):
        ops.cla_fwd_packed(q, q, q, [1, 4, 10])
    out = ops.causal_linear_attention_packed(q, q, q, torch.tensor([0, 4, 10], dtype=torch.int32, device=cuda))
    assert out.shape == q.shape and torch.isfinite(out.float()).all()
    lib = _lib.load()
    cu = ops.SeqOffsets([0, 4, 10], device=cuda)
    p = lambda t: _lib.dev(t)
    z = torch.empty(10, H, device=cuda)
    # a row stride the route cannot take: final state wanted on a stride that is no multiple of 8
    assert lib.cwlt_causal_linear_fwd_packed(p(q), p(q), p(q), p(q), p(z), p(cu.dev), 2, H, 64, 132, 132, 132, 128, 1e-6,
                                             p(z), 1, None) == 1001
    assert lib.cwlt_causal_linear_fwd_packed(p(q), p(q), p(q), p(q), p(z), p(cu.dev), 2, H, 64, 64, 128, 128, 128, 1e-6,
                                             None, 1, None) == 1001       # ld < H * 64
