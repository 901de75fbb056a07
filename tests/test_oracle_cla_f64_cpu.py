"""CPU pin of oracle/cla_f64.py, the reference, measure and bounds of tests/test_cla_f64_gpu.py: the reference forms agree,
the row terms equal a brute-force L x L x 64 evaluation, the f64 emulation of the MFMA kernels' bf16 roundings (and torch's
own f32 chain as a stand-in for the f32 and generic kernels) stays inside every bound the GPU test applies, and every
"teeth" mutant falls outside its bound by TEETH = 5.  No kernel runs here.  Run with -s for the figures."""
import pytest
import torch

from oracle import cla as ocla
from oracle import cla_f64 as o

KINDS = ("randn", "x3", "vmean", "eps")
NAMES = ("out", "dq", "dk", "dv")
_CACHE = {}


def case(kind, N, L, H, seed=1):
    key = (kind, N, L, H, seed)
    if key not in _CACHE:
        x = o.make_inputs(kind, N, L, H, seed)
        ref = o.reference(*x, kf_round=o.rb)
        _CACHE[key] = (x, ref, o.analyse(ref))
    return _CACHE[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,L,H", [(2, 96, 2), (1, 200, 1), (1, 1, 1), (3, 65, 1)])
def test_reference_forms_agree(kind, N, L, H):
    """chunked + autograd (the reference), quadratic + autograd, the explicit L x L formulas and the chunked scans of
    emulate_mfma with the rounding switched off: out, dq, dk, dv to 1e-11 of each row's denominator (or of its operand
    term: at L = 1, c_00 = z dout . (v - out) cancels inside the one term, in f64 too); zinv, dden, state."""
    x, ref, t = case(kind, N, L, H)
    xd = [a.double() for a in x]
    forms = {"quadratic": ocla.cla_grads(*xd, fn=ocla.cla_quadratic), "explicit": o.explicit_grads(*x)}
    if kind == "eps":
        del forms["quadratic"]      # oracle.cla evaluates elu(x) + 1 as (exp(x) - 1) + 1: eight digits at k = -20
    for form in ("pair", "sweep"):
        em = o.emulate_mfma(*x, form, r=lambda a: a)
        forms["scan " + form] = tuple(em[n] for n in NAMES)
        assert ((em["zinv"] - ref["zinv"]).abs() / ref["zinv"]).max().item() < 1e-12
        assert ((em["dden"] - ref["dden"]).abs() / t["dden"].clamp_min(1e-300)).max().item() < 1e-12
    for label, got in forms.items():
        for n, g in zip(NAMES, got):
            assert o.row_ratio(g, ref[n], torch.maximum(t["den_" + n], t["E_" + n])).max().item() < 1e-11, (label, n)
    em = o.emulate_mfma(*x, "sweep")            # its final state sums the rounded phi(k), as ref's does with kf_round
    assert (em["fin_S"] - ref["fin_S"]).abs().max().item() <= 1e-12 * ref["fin_S_abs"].max().item()
    assert (em["fin_z"] - ref["fin_z"]).abs().max().item() <= 1e-12 * ref["fin_z"].max().item()


@pytest.mark.parametrize("kind", KINDS)
def test_row_terms_equal_brute_force(kind):
    x, ref, t = case(kind, 2, 96, 2)
    brute = o.row_terms_brute(ref)
    for n in NAMES:
        assert ((t[n] - brute[n]).abs() / brute[n]).max().item() < 1e-12, n
    # the uncancelled norm is never below the row itself (up to rounding): it is a root-sum-square of the terms of a sum
    # of at most 96 of them
    for n in ("out", "dv"):
        assert (ref[n].norm(dim=-1) <= 96 ** 0.5 * t[n] * (1 + 1e-12)).all()


def test_operand_terms_against_the_definition():
    """E(dq), E(dk) by the L x L x 64 x 64 definition at L = 20."""
    x = o.make_inputs("vmean", 1, 20, 1, 3)
    ref = o.reference(*x)
    e = o.operand_terms(ref)
    q, k, v, d, out = (ref[n][0, :, 0] for n in ("q", "k", "v", "dout", "out"))
    z = ref["zinv"][0, :, 0, None]
    Q, K, g = o.phi(q), o.phi(k), d * z
    tril = torch.tril(torch.ones(20, 20, dtype=torch.float64))
    S = torch.einsum("ij,je,jm->iem", tril, K, v)
    S2 = torch.einsum("ij,je,jm->iem", tril, K ** 2, v ** 2)
    do2 = (g ** 2 * out ** 2).sum(-1, keepdim=True)
    e_dq = (o.dphi(q) ** 2 * (torch.einsum("im,iem->ie", g ** 2, S ** 2 + S2) + K.cumsum(0) ** 2 * do2)).sum(-1).sqrt()
    R = torch.einsum("ij,ie,im->jem", tril, Q, g)
    R2 = torch.einsum("ij,ie,im->jem", tril, Q ** 2, g ** 2)
    R3 = torch.einsum("ij,ie->je", tril, Q ** 2 * do2)
    e_dk = (o.dphi(k) ** 2 * (torch.einsum("jm,jem->je", v ** 2, R ** 2 + R2) + R3)).sum(-1).sqrt()
    assert ((e["dq"][0, :, 0] - e_dq).abs() / e_dq).max().item() < 1e-12
    assert ((e["dk"][0, :, 0] - e_dk).abs() / e_dk).max().item() < 1e-12


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,L,H", [(3, 65, 1), (1, 200, 2), (1, 1024, 2)])
@pytest.mark.parametrize("form", ["pair", "sweep"])
def test_emulated_roundings_stay_inside_the_bounds(kind, N, L, H, form):
    """Nothing but the bf16 roundings of the MFMA forms, in f64: every row, zinv, dden and column sum inside the bound
    the GPU test applies to that form."""
    x, ref, t = case(kind, N, L, H)
    name = "mfma" if form == "pair" else "sweep"
    em = o.emulate_mfma(*x, form)
    b = o.bounds(name, ref, t, L)
    worst = {}
    for n in NAMES:
        worst[n] = (o.row_ratio(em[n], ref[n], t["den_" + n]) / b[n]).max().item()
    worst["zinv"] = ((em["zinv"] - ref["zinv"]).abs() / ref["zinv"]).max().item() / o.zinv_bound(name, L)
    worst["dden"] = ((em["dden"] - ref["dden"]).abs() / t["dden"]).max().item() / o.dden_bound(name, L)
    # column sums: what the kernel adds up against the sum of the stored values
    for i, n in enumerate(("dq", "dk", "dv")):
        stored = em[n].sum(1)                                        # (N, H, 64)
        sabs, rss = em[n].abs().sum(1), (em[n] ** 2).sum(1).sqrt()
        allow = o.colsum_bound(L) * sabs + (4 * 2 * o.U16 * rss if form == "pair" and n != "dv" else 0)
        worst["cs_" + n] = ((em["cs"][i] - stored).abs() / allow.clamp_min(1e-300)).max().item()
    print("\n  %s %s (%d, %d, %d): %s" % (form, kind, N, L, H, "  ".join("%s %.2f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,L,H", [(3, 65, 1), (1, 1024, 1)])
def test_torch_f32_chain_stays_inside_the_f32_and_generic_bounds(kind, N, L, H):
    """torch's own f32 arithmetic (chunked form + autograd) as a stand-in for the f32 kernels, and the same on bf16 inputs
    with the output and the gradients rounded to bf16 (out before the backward reads it) for the generic bf16 form."""
    for form, dtype in (("f32", torch.float32), ("generic", torch.bfloat16)):
        x = o.make_inputs(kind, N, L, H, 2, dtype)
        ref = o.reference(*x)
        t = o.analyse(ref)
        b = o.bounds(form, ref, t, L)
        q, k, v, d = (a.float().requires_grad_(True) for a in x)
        out = o.cla_chunked(q, k, v, chunk=32) if kind != "eps" else ocla.cla_chunked(q, k, v, chunk=32)
        if form == "generic":
            out = out + (out.detach().bfloat16().float() - out.detach())     # the stored value, straight through
        out.backward(d.detach())
        got = (out.detach(), q.grad, k.grad, v.grad)
        worst = {}
        for n, g in zip(NAMES, got):
            g = g.bfloat16() if form == "generic" else g
            worst[n] = (o.row_ratio(g, ref[n], t["den_" + n]) / b[n]).max().item()
        print("\n  %s stand-in %s (%d, %d, %d): %s" % (form, kind, N, L, H, "  ".join("%s %.2f" % kv for kv in worst.items())))
        assert max(worst.values()) <= 1.0, (form, worst)


def test_no_row_needs_a_floor():
    """The measure has no tensor-wide floor: with max(|ref row|, T_row) as the denominator the reference alone leaves no
    row without one (den > 0 on every row of every input), so no row class takes a floor: share 0 <= 2 %."""
    for kind in KINDS:
        _, ref, t = case(kind, 1, 1024, 2)
        for n in NAMES:
            assert (t["den_" + n] > 0).all(), (kind, n)
            assert (ref[n].norm(dim=-1) <= t["den_" + n]).all()


@pytest.mark.parametrize("mutant,kind,shape,segs,tensors,rows", o.MUTANTS)
@pytest.mark.parametrize("form", ["pair", "sweep"])
def test_mutants_fall_outside_the_bound(mutant, kind, shape, segs, tensors, rows, form):
    """The emulated kernel is inside the bound against the right reference and at least TEETH x the bound away from the
    reference with one wrong ingredient, in the rms over the rows that ingredient feeds."""
    x, ref, t = case(kind, *shape)
    L = shape[1]
    name = "mfma" if form == "pair" else "sweep"
    em = o.emulate_mfma(*x, form)
    b = o.bounds(name, ref, t, L)
    mut = o.mutant_reference(*x, mutant, segments=segs)
    for n in tensors:
        inside = (o.row_ratio(em[n], ref[n], t["den_" + n]) / b[n]).max().item()
        miss = o.teeth(em[n], mut[n], t["den_" + n], b[n], rows)
        print("\n  %s %s %s: inside %.2f, mutant %.1f x the bound" % (mutant, form, n, inside, miss))
        assert inside <= 1.0 and miss >= o.TEETH, (mutant, n, inside, miss)
    if mutant == "eps0":
        r = ((em["zinv"] - mut["zinv"]).abs() / mut["zinv"])[:, rows].max().item() / o.zinv_bound(name, L)
        assert r >= o.TEETH


def test_the_tensor_wide_rule_misses_two_of_the_mutants():
    """What the first-round rule (max |got - ref| <= 2^-7 max(1, max |ref|), tests/test_cla_gpu.py) lets through, on
    test_cla_bf16_io's inputs at (1, 1024, 2): the dropped diagonal in dq and dk, and the zeroed tail in dk and dv."""
    g = torch.Generator().manual_seed(11)
    x = [torch.randn(1, 1024, 2, 64, generator=g).bfloat16() for _ in range(4)]
    ref = o.reference(*x)
    for mutant, tensors in (("diag", ("dq", "dk")), ("tail", ("dk", "dv"))):
        mut = o.mutant_reference(*x, mutant)
        for n in tensors:
            err = (mut[n] - ref[n]).abs().max().item()
            assert 0 < err <= 2.0 ** -7 * max(1.0, ref[n].abs().max().item()), (mutant, n, err)
