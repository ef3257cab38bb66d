"""The conjugate-gradient entry points of include/cine_hip.h (csrc/pack_kernels.hip, train_kernels.hip and the solver of fft_kernels.hip) called
one by one through the C ABI, shape by shape, against float64 references on the CPU.

Entry points
  V  vectors of n floats: cine_dot, cine_axpby_dev (num / den, num alone, softplus(lambda)), cine_axpby_lam (kinds 0 - 3, a NULL or given),
     cine_cg_step, cine_cg_step_pd, cine_cg_step_pd2, cine_cg_adjoint_step, cine_cg_adjoint_finish and the size functions
  F  one iteration with the operator inside: cine_normal_op_pd + cine_cg_step_pd chained, cine_normal_op_cg_fused, cine_normal_op_cg_fused_t
  S  the whole solve: cine_conj_grad, cine_conj_grad_rec (p_rec, rr_rec, pd_rec), cine_conj_grad_ws_bytes

References: float64 on the CPU from the header's definitions and cinenet.py:121-171, inputs the float32 values the kernel sees, widened.
Dot products are plain sums, softplus is log1p(exp(x)) without the shortcut above 20, H = A^H M A + softplus(lambda) I is the composition
ref_normal_op of test_transform_kernels.py, the iteration is the literal one (ref_cg) with every p_k, rr_k, pd_k kept, one reverse step of
the adjoint is the header's three formulas (ref_adjoint_step).  The CPU tests (no gpu mark) pin ref_cg to the oracle's ConjGrad / HOperator
and the adjoint recurrence, run over all iterations, to float64 autograd of the oracle's ConjGrad (which detaches alpha and beta), at 1e-10.

The bar.  The one-step entry points (V, F) are not iterative: vectors meet kernel_sweep.BAR = 1e-5 of the reference's peak; scalars are
measured against their cancellation-free scale (sum |a_i b_i| for a dot, the reference itself for r.r and p.Hp) and meet BAR up to
LONG_REDUCTION summed terms, kernel_sweep._bar with torch's own float32 result above.  The chained quantities of a whole solve (x, every p_k
against its own peak, every rr_k, every pd_k) are measured against the float64 iteration of the same count at max(BAR, 2 x e32), e32 the error
of the SAME iteration run in torch float32 on the CPU for that case and quantity; a CPU test holds every e32 to BAR_CAP / 2.  Two identities
on the device's own records do not depend on the conditioning and are held at BAR: x = x0 + sum_k (rr_k / pd_k) p_k and
pd_k = <p_k, H p_k>, both evaluated in float64 from the recorded float32 values.  The yardstick also decides which masks a whole solve
is measured on (see S_CASES): a mask per frame carries every (lambda, iters) pair; one shared row only the pairs whose late directions
stay under the cap in float32 on the CPU; "all" and "none" make H a multiple of the identity, where only the first, exact step is well
posed -- they run without an iteration and with that one step (IDENTITY_CASES), held to BAR.  Largest e32 over the cases, on the CPU:
3.5e-6 for x, 4.2e-5 for a p_k (lambda = 20.1, the sixth direction), 5.0e-6 for an rr_k, 2.1e-6 for a pd_k.

Every GPU case checks: the error; a NaN prefill of every pure output; guard floats around every output and every in-place operand; a
workspace of exactly the size asked for, prefilled with 0xFF bytes, its sentinel tail intact; the inputs declared const bit-unchanged; a
second identical call gives the same bits.  Group V runs at storage offsets of 0 and 1 float and must give the same bits at both.
Refusals are decided on the host before any launch: return code, message, operands untouched.  DESIGN.md section 4d has the measured worst
error / bar per entry point and the mutations the sweep was tried against.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err
from kernel_sweep import (BAR, BAR_CAP, EINVAL, EUNSUPPORTED, EWORKSPACE, Call, L, Worst, _bar, at_offsets, cap_samples, case_id, check,
                          hash_case, ptr, refused, same_bits, stream, sweep, twice)
from test_transform_kernels import LAMBDAS, _rand, cplx, make_mask, pairs, ref_normal_op, ref_softplus

PIN = 1e-10                                    # float64 restatement against the float64 oracle


# ================================================================== float64 references (CPU)
def rdot(a, b):
    """The real inner product over interleaved (re, im) (cinenet.py:148), a plain sum; real or complex tensors."""
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return torch.dot(a.flatten(), b.flatten())


def ref_cg(x0, rhs, S, mask, lam, iters, rhs_is_ref=False):
    """cinenet.py:136-171, the literal iteration (test_hip_parity.py's restatement) in the precision of its inputs: x0, rhs (b, t, h, w)
    complex, S (b, c, h, w), mask (b, t, h).  Returns x, [p_k], [rr_0 .. rr_iters], [pd_k]."""
    H = lambda z: ref_normal_op(z, S, mask, lam)
    b = rhs + ref_softplus(lam) * x0 if rhs_is_ref else rhs          # cinenet.py:106-107
    x = x0
    r = b - H(x)
    p = r.clone()
    rr = rdot(r, r)
    P, RR, PD = [], [rr], []
    for _ in range(iters):
        d = H(p)
        pd = rdot(p, d)
        P.append(p); PD.append(pd)
        al = rr / pd
        x = x + al * p
        r = r - al * d
        rn = rdot(r, r)
        p = r + (rn / rr) * p
        rr = rn
        RR.append(rr)
    return x, P, RR, PD


def ref_cg_step(x, r, p, d, rr_old, pd=None):
    """One iteration after d = H p (cinenet.py:155-169) on float64 tensors: x, r, p, rr_new, pd."""
    pd = rdot(p, d) if pd is None else pd
    al = rr_old / pd
    x = x + al * p
    r = r - al * d
    rn = rdot(r, r)
    return x, r, r + (rn / rr_old) * p, rn, pd


def ref_adjoint_step(gp, q, gx, hg, pk, rr, pd, rr_new):
    """The header's reverse step: gp <- (rr_new / rr) gp + (rr / pd) gx - (rr / pd) hg, s = <q, p_k> of the OLD q, q <- q + gp."""
    s = rdot(q, pk)
    gp = (rr_new / rr) * gp + (rr / pd) * gx - (rr / pd) * hg
    return gp, q + gp, s


def ref_cg_adjoint(gx, x0, P, RR, PD, H):
    """ConjGradFn's recurrence from the last iteration to the first: gb = q_0, gx0 = gx - H gb, gv - <gb, x0>."""
    q, gp, gv = torch.zeros_like(gx), torch.zeros_like(gx), 0.0
    for k in reversed(range(len(P))):
        gp, q, s = ref_adjoint_step(gp, q, gx, H(q), P[k], RR[k], PD[k], RR[k + 1])
        gv = gv - (RR[k] / PD[k]) * s
    return gx - H(q), q, gv - rdot(q, x0)


def dot_partials(a, b):
    """cine_dot's first stage: 256 workgroups of 256 threads walk the vector with a stride of 65 536, so element i is summed by workgroup
    (i // 256) % 256.  Float64 sums."""
    n = a.numel()
    part = torch.zeros(256, dtype=torch.float64)
    part.index_add_(0, (torch.arange(n) // 256) % 256, a.double() * b.double())
    return part


# ================================================================== case lists
V_N = [1, 2, 3, 255, 256, 257, 65_535, 65_536, 65_537, 200_003]
OFFS = (0, 1)                                  # storage offsets in floats: plain float arrays, the header asks for no alignment
KINDS = [0, 1, 2, 3]
FINISH_ITERS = [0, 1, 2, 6]
LAM_ITERS = [(-30.0, 3), (-1.3, 4), (-1.3, 6), (0.5413, 4), (0.5413, 6), (19.9, 2), (20.1, 2), (20.1, 6), (25.0, 1)]
H200 = 200
SHAPE_AXES = dict(c=[6, 10, 11, 16, 21, 31], w=[1, 3, 5, 7, 12], b=[1, 2], t=[1, 2, 3], mask=["frame", "one", "all", "none"])


def _finish_cases(cases):
    """"none" only where H is well away from singular (softplus(lambda) >= 0.2); t capped so that one float64 reference stays fast."""
    for c in cases:
        if c["mask"] == "none" and ref_softplus(c["lam"]) < 0.2:
            c["mask"] = "frame"
        c["t"] = cap_samples(c["t"], c["b"] * c["c"] * H200 * c["w"], 400_000)
    return cases


def _f(c, w, b, t, mask, lam):
    return dict(c=c, w=w, b=b, t=t, mask=mask, lam=lam)


def _s(c, w, b, t, mask, rhs_is_ref, lam, iters):
    return dict(c=c, w=w, b=b, t=t, mask=mask, rhs_is_ref=rhs_is_ref, lam=lam, iters=iters)


F_CASES = sweep(41, dict(SHAPE_AXES, lam=LAMBDAS), 12)
# the crossings an axis-by-axis walk does not promise: every lambda on b = 2 with a ragged last column tile, one coil group more than a
# multiple of 8 workgroups (idle workgroups), a full grid (2 column tiles x 4 coil groups)
F_CASES += [_f(*a) for a in [(11, 3, 2, 2, "frame", -30.0), (6, 7, 2, 1, "one", -1.3), (16, 12, 2, 2, "frame", 0.5413), (21, 1, 2, 3, "all", 19.9),
                             (31, 7, 2, 1, "frame", 20.1), (10, 3, 2, 2, "none", 25.0), (16, 7, 1, 2, "frame", 0.5413), (6, 12, 1, 1, "one", 20.1)]]
F_CASES = _finish_cases(F_CASES)

# Group S.  Which masks a whole solve can be measured on is decided by the float64 reference's own float32 twin (e32, below), not by the
# device: with the maps normalised, "all" and "none" make H a multiple of the identity, the first step is exact and every later one
# divides rounding residue by rounding residue (e32 of p_1 is 1e2 and more); with "one" (one row, the same in every frame) the residual
# collapses so fast that the late directions pass the cap (e32 of the last p_k: 9e-5 .. 8e-2 at (-1.3, 6), (0.5413, 4), (0.5413, 6),
# (19.9, 2), (20.1, 2), (20.1, 6); 4e-5 and less at the three pairs of ONE_OK).  So "frame" carries every (lambda, iters) pair, "one"
# the pairs of ONE_OK, and "all" / "none" run where the iteration is well posed: without an iteration (ZERO_ITERS_CASES) and with
# the one exact step (IDENTITY_CASES, a test of its own).
ONE_OK = {(-30.0, 3), (-1.3, 4), (25.0, 1)}
_S = sweep(43, dict({k: v for k, v in SHAPE_AXES.items() if k != "mask"}, rhs_is_ref=[0, 1], li=list(range(len(LAM_ITERS)))), 12)
S_CASES = [dict(c=c["c"], w=c["w"], b=c["b"], t=c["t"], mask="one" if LAM_ITERS[c["li"]] in ONE_OK and i % 2 == 0 else "frame", rhs_is_ref=c["rhs_is_ref"],
                lam=LAM_ITERS[c["li"]][0], iters=LAM_ITERS[c["li"]][1]) for i, c in enumerate(_S)]
S_CASES += [_s(*a) for a in [(6, 5, 1, 2, "one", 1, -30.0, 3), (11, 3, 2, 2, "one", 0, -1.3, 4), (16, 7, 2, 1, "frame", 1, -1.3, 6),
                             (10, 12, 2, 2, "frame", 0, 0.5413, 4), (21, 3, 2, 3, "frame", 1, 0.5413, 6), (31, 1, 2, 1, "frame", 0, 19.9, 2),
                             (6, 7, 2, 2, "frame", 1, 20.1, 2), (11, 5, 1, 3, "frame", 0, 20.1, 6), (16, 12, 2, 1, "one", 1, 25.0, 1),
                             (31, 3, 1, 2, "frame", 0, 25.0, 1)]]
S_CASES = _finish_cases(S_CASES)
WS_CASE = _s(11, 7, 2, 2, "frame", 1, 0.5413, 4)           # cine_conj_grad with its workspace 16 bytes past a 256-byte boundary
ZERO_ITERS_CASES = [_s(6, 3, 1, 2, "all", 0, 0.5413, 0), _s(11, 7, 2, 1, "none", 1, 20.1, 0), _s(10, 5, 2, 2, "frame", 1, -30.0, 0)]
IDENTITY_CASES = [_s(6, 3, 1, 2, "all", 0, 0.5413, 1), _s(11, 7, 2, 1, "none", 1, 20.1, 1), _s(16, 5, 2, 2, "all", 1, -30.0, 1), _s(10, 12, 1, 1, "none", 0, -1.3, 1)]


def nz_of(c):
    return -(-c["c"] // 5)


def workgroups(c):
    """Coil groups x column tiles per frame; the grid rounds them up to a multiple of 8."""
    return -(-c["w"] // 5) * nz_of(c)


# ================================================================== inputs and references per case (CPU; shared by the tests)
def cg_vectors(n):
    """x, r, p, d = noise + 3 p (the existing test's well-conditioned p.d) and rr_old = the float32 r.r."""
    x, r, p, z = (_rand(n * 11 + i, n) for i in range(4))
    d = z + 3 * p
    rr_old = (r.double() * r.double()).sum().float().reshape(1)
    return x, r, p, d, rr_old


def adjoint_vectors(n):
    gp, q, gx, hg, pk = (_rand(n * 13 + i, n) for i in range(5))
    rs = np.random.RandomState(n % 1000 + 5)
    rr, pd, rr_new = (torch.tensor([v], dtype=torch.float32) for v in rs.uniform(0.5, 2.0, 3))      # rr > 0, pd > 0
    return gp, q, gx, hg, pk, rr, pd, rr_new


def shape_data(c, seed):
    """Maps normalised to sum_c |S_c|^2 = 1 (cond(H) <= (1 + v) / v), a mask per frame, three image-sized vectors."""
    b, t, C, w = c["b"], c["t"], c["c"], c["w"]
    S = _rand(seed, b, C, H200, w, 2)
    S = (S / S.pow(2).sum(dim=(1, 4), keepdim=True).sqrt()).contiguous()
    mask = make_mask(seed + 1, b * t, H200, c["mask"]).view(b, t, H200)
    return S, mask, [_rand(seed + 2 + i, b, t, H200, w, 2) for i in range(3)]


@functools.lru_cache(maxsize=None)
def _f_ref(key):
    c = dict(key)
    S, mask, (x, r, z) = shape_data(c, hash_case(c))
    p = (r + 0.5 * z).contiguous()                               # a direction that is not the residual
    rr_old = (r.double() * r.double()).sum().float().reshape(1)
    d = pairs(ref_normal_op(cplx(p), cplx(S), mask, c["lam"]))
    ref = ref_cg_step(x.double(), r.double(), p.double(), d, rr_old.double()[0])
    return dict(S=S, mask=mask, x=x, r=r, p=p, rr_old=rr_old, ref=ref)


def f_ref(c):
    return _f_ref(tuple(sorted(c.items())))


def _errors(got, ref):
    """The error of every chained quantity of a solve against the float64 one: x and each p_k against their own peak, rr_k and pd_k
    against the reference value (sums of non-negative / positive-definite terms)."""
    x, P, RR, PD = got
    x64, P64, RR64, PD64 = ref
    e = {"x": rel_err(pairs(x), pairs(x64))}
    e["p"] = [rel_err(pairs(a), pairs(b)) for a, b in zip(P, P64)]
    e["rr"] = [abs(float(a) - float(b)) / float(b) for a, b in zip(RR, RR64)]
    e["pd"] = [abs(float(a) - float(b)) / float(b) for a, b in zip(PD, PD64)]
    return e


@functools.lru_cache(maxsize=None)
def _s_ref(key):
    """Inputs, the float64 iteration and e32: the error of the same iteration in torch float32 on the CPU."""
    c = dict(key)
    S, mask, (x0, rhs, _) = shape_data(c, hash_case(c))
    ref = ref_cg(cplx(x0), cplx(rhs), cplx(S), mask, c["lam"], c["iters"], bool(c["rhs_is_ref"]))
    c64 = lambda v: torch.view_as_complex(v.contiguous())
    run32 = ref_cg(c64(x0), c64(rhs), c64(S), mask, c["lam"], c["iters"], bool(c["rhs_is_ref"]))
    assert run32[0].dtype == torch.complex64 and ref[0].dtype == torch.complex128
    return dict(S=S, mask=mask, x0=x0, rhs=rhs, ref=ref, e32=_errors(run32, ref))


def s_ref(c):
    return _s_ref(tuple(sorted(c.items())))


def chained_bar(e32):
    return max(BAR, 2 * e32)


# ================================================================== CPU tests: the references, the case lists, the e32 cap
def _oracle_block(lam, iters):
    from oracle import cinenet_ref as C
    blk = C.CineNetBlock(torch.nn.Identity(), iters, "XF", True).double()
    with torch.no_grad():
        blk.lambda_reg.fill_(float(np.float32(lam)))
    return blk


ORACLE_CASES = [(1, 2, 6, 200, 5, "frame", 0.5413, 4), (2, 2, 11, 200, 3, "frame", -1.3, 6), (2, 3, 3, 12, 7, "one", 0.5413, 3), (1, 1, 2, 9, 4, "frame", 2.5, 2)]


def _oracle_data(case):
    b, t, C, h, w, kind, lam, iters = case
    seed = sum(case[:5]) + iters
    S = _rand(seed, b, C, h, w, 2)
    S = S / S.pow(2).sum(dim=(1, 4), keepdim=True).sqrt()
    mask = make_mask(seed + 1, b * t, h, kind).view(b, t, h)
    x0, rhs, g = (_rand(seed + 2 + i, b, t, h, w, 2) for i in range(3))
    o = lambda v: v.double().unsqueeze(2)                     # (b, t, 1, h, w, 2)
    return S, mask, x0, rhs, g, o, S.double().unsqueeze(1), mask.double()[:, :, None, :, None, None]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=str)
def test_reference_iteration_is_the_oracles(case):
    lam, iters = case[6:]
    S, mask, x0, rhs, g, o, So, mo = _oracle_data(case)
    blk = _oracle_block(lam, iters)
    assert rel_err(pairs(ref_normal_op(cplx(x0), cplx(S), mask, lam)), blk.HOperator(o(x0), mo, So).squeeze(2)) < PIN
    x, P, RR, PD = ref_cg(cplx(x0), cplx(rhs), cplx(S), mask, lam, iters)
    assert len(P) == iters and len(RR) == iters + 1 and len(PD) == iters
    assert rel_err(pairs(x), blk.ConjGrad(o(x0), o(rhs), mo, So, iters).squeeze(2)) < PIN
    v = ref_softplus(lam)
    xr = ref_cg(cplx(x0), cplx(rhs), cplx(S), mask, lam, iters, rhs_is_ref=True)[0]
    assert rel_err(pairs(xr), blk.ConjGrad(o(x0), o(rhs) + v * o(x0), mo, So, iters).squeeze(2)) < PIN
    # one iteration of ref_cg is ref_cg_step
    H = lambda z: ref_normal_op(z, cplx(S), mask, lam)
    x1 = ref_cg_step(pairs(cplx(x0)), pairs(P[0]), pairs(P[0]), pairs(H(P[0])), RR[0])[0]
    assert rel_err(x1, pairs(ref_cg(cplx(x0), cplx(rhs), cplx(S), mask, lam, 1)[0])) < PIN


@pytest.mark.parametrize("case", ORACLE_CASES, ids=str)
def test_reference_adjoint_recurrence_is_autograd_of_the_oracle(case):
    lam, iters = case[6:]
    S, mask, x0, rhs, g, o, So, mo = _oracle_data(case)
    blk = _oracle_block(lam, iters)
    xo, bo = o(x0).requires_grad_(True), o(rhs).requires_grad_(True)
    with torch.enable_grad():
        (o(g) * blk.ConjGrad(xo, bo, mo, So, iters)).sum().backward()
    dv = float(blk.lambda_reg.grad) / float(torch.sigmoid(blk.lambda_reg.detach()))          # d softplus / d lambda
    _, P, RR, PD = ref_cg(cplx(x0), cplx(rhs), cplx(S), mask, lam, iters)
    gx0, gb, gv = ref_cg_adjoint(cplx(g), cplx(x0), P, RR, PD, lambda z: ref_normal_op(z, cplx(S), mask, lam))
    assert rel_err(pairs(gx0), xo.grad.squeeze(2)) < PIN
    assert rel_err(pairs(gb), bo.grad.squeeze(2)) < PIN
    assert abs(float(gv) - dv) <= PIN * max(abs(dv), float(rdot(gb, cplx(x0)).abs()))


def test_dot_partials_follow_the_grid_stride():
    a, b = _rand(1, 70_000), _rand(2, 70_000)
    part = dot_partials(a, b)
    assert abs(float(part.sum()) - float((a.double() * b.double()).sum())) < 1e-9
    assert abs(float(part[1]) - float((a[256:512].double() * b[256:512].double()).sum() + (a[65_792:66_048].double() * b[65_792:66_048].double()).sum())) < 1e-12


def test_step_cases_have_a_well_conditioned_alpha():
    for n in V_N:
        _, _, p, d, rr_old = cg_vectors(n)
        prod = p.double() * d.double()
        assert abs(float(prod.sum())) >= 0.5 * float(prod.abs().sum()), n
        assert float(rr_old) > 0
        rr, pd, rr_new = adjoint_vectors(n)[5:]
        assert float(rr) > 0 and float(pd) > 0 and float(rr_new) > 0


def test_case_lists_reach_every_value_and_crossing():
    for cases, what in ((F_CASES, "cg_fused"), (S_CASES, "conj_grad / conj_grad_rec")):
        for k, vals in SHAPE_AXES.items():
            if k != "mask":
                assert {c[k] for c in cases} == set(vals), (what, k)
        assert {c["lam"] for c in cases} == set(LAMBDAS), what            # both sides of the softplus switch at 20
        assert 3 * sum(c["b"] == 2 for c in cases) >= len(cases), what
        assert any(workgroups(c) % 8 != 0 for c in cases) and any(workgroups(c) % 8 == 0 for c in cases), what
        assert any(c["w"] % 5 != 0 and c["b"] == 2 for c in cases), what
        assert {nz_of(c) for c in cases} == {2, 3, 4, 5, 7}, what                 # ragged and full coil groups
    for c in F_CASES + S_CASES + ZERO_ITERS_CASES + IDENTITY_CASES:
        assert c["mask"] != "none" or ref_softplus(c["lam"]) >= 0.2, c
    assert {c["mask"] for c in F_CASES} == set(SHAPE_AXES["mask"])
    assert {c["mask"] for c in S_CASES} == {"frame", "one"} and {c["mask"] for c in ZERO_ITERS_CASES + IDENTITY_CASES} >= {"all", "none"}
    assert {(c["lam"], c["iters"]) for c in S_CASES if c["mask"] == "frame"} == set(LAM_ITERS)    # cine_conj_grad and cine_conj_grad_rec run on every S case
    assert {(c["lam"], c["iters"]) for c in S_CASES if c["mask"] == "one"} == ONE_OK
    assert {(c["rhs_is_ref"], c["lam"] > 20) for c in S_CASES} == {(0, False), (0, True), (1, False), (1, True)}
    assert all(c["iters"] == 0 for c in ZERO_ITERS_CASES) and {c["rhs_is_ref"] for c in ZERO_ITERS_CASES} == {0, 1}
    assert all(c["iters"] == 1 for c in IDENTITY_CASES) and {c["rhs_is_ref"] for c in IDENTITY_CASES} == {0, 1}
    for c in [WS_CASE] + [c for c in S_CASES if c["mask"] == "frame" and c["b"] == 2 and c["t"] >= 2][:3]:
        frames = s_ref(c)["mask"].view(-1, H200)
        assert c["mask"] == "frame" and not torch.equal(frames[0], frames[1]) and not torch.equal(frames[0], frames[-1])      # frames carry different masks, across b too


@pytest.mark.parametrize("c", S_CASES + [WS_CASE], ids=case_id)
def test_float32_yardstick_stays_under_the_cap(c):
    """e32 <= BAR_CAP / 2 for every case and quantity, so the bar max(BAR, 2 x e32) never passes BAR_CAP."""
    d = s_ref(c)
    e = d["e32"]
    worst = {k: (max(v) if isinstance(v, list) else v) for k, v in e.items()}
    print(case_id(c), " ".join(f"e32({k}) = {v:.2e}" for k, v in worst.items()))
    assert all(float(v) > 0 for v in d["ref"][3]) and all(float(v) > 0 for v in d["ref"][2])
    for k, v in worst.items():
        assert v <= BAR_CAP / 2, (k, v)


# ================================================================== GPU harness
gpu = pytest.mark.gpu
WORST = Worst()
_record = WORST.record


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    yield torch.device("cuda:0")
    if WORST:
        WORST.report()


def _scalar_err(got, ref, scale=None):
    return abs(float(got) - float(ref)) / float(ref if scale is None else scale)


# ================================================================== V: vectors of n floats
@gpu
def test_size_functions(dev):
    lib = L()
    assert lib.cine_dot_ws_bytes() == 256 * 4 and lib.cine_cg_ws_bytes() == 2 * 256 * 4 and lib.cine_cg_adjoint_part_floats() == 256
    for c in F_CASES + S_CASES:
        b, t, C, w = c["b"], c["t"], c["c"], c["w"]
        nb = -(-workgroups(c) // 8) * 8 * b * t
        dc = lib.cine_image_dc_ws_bytes(b, t, C, H200, w)
        assert dc == nz_of(c) * b * t * H200 * w * 8
        assert lib.cine_cg_fused_ws_bytes(b, t, C, H200, w) == (nb + 256) * 4
        # the coil-group sums, one p.Hp partial per workgroup, two r.r arrays, the round-up to 256 bytes, {p, r} pairs and p
        assert lib.cine_conj_grad_ws_bytes(b, t, C, H200, w) == dc + (nb + 512) * 4 + 256 + b * t * H200 * w * (16 + 8)


@gpu
@pytest.mark.parametrize("n", V_N)
def test_dot(dev, n):
    a, b = _rand(n * 7 + 1, n), _rand(n * 7 + 2, n)
    prod = a.double() * b.double()
    ref, scale = float(prod.sum()), float(prod.abs().sum())
    bar = _bar(abs(float(torch.dot(a, b)) - ref) / scale, n)

    def body(k):
        ad, bd, o, ws = k.inp(a), k.inp(b), k.out((1,)), k.ws(L().cine_dot_ws_bytes())
        check(L().cine_dot(ad.data_ptr(), bd.data_ptr(), n, o.ptr(), ws.ptr(), stream()), "cine_dot")
        return [o.t]
    got, = at_offsets(dev, OFFS, body, "cine_dot")
    _record("cine_dot", _scalar_err(got, ref, scale), bar, n)
    got, = at_offsets(dev, OFFS, lambda k: body_same(k, a, n), "cine_dot")           # a.a: both operands one array
    sq = float((a.double() * a.double()).sum())
    _record("cine_dot", _scalar_err(got, sq), _bar(abs(float(torch.dot(a, a)) - sq) / sq, n), n)


def body_same(k, a, n):
    ad, o, ws = k.inp(a), k.out((1,)), k.ws(L().cine_dot_ws_bytes())
    check(L().cine_dot(ad.data_ptr(), ad.data_ptr(), n, o.ptr(), ws.ptr(), stream()), "cine_dot")
    return [o.t]


@gpu
@pytest.mark.parametrize("n", V_N)
def test_axpby_dev(dev, n):
    """out = a + sign * s * b with s = num / den, num, or softplus(lambda); the lambda form also with a = 0, where the output is s * b
    alone and shows s at every lambda; out == a and out == b give the bits of the out-of-place call."""
    a, b = _rand(n * 5 + 1, n), _rand(n * 5 + 2, n)
    num, den = torch.tensor([1.7]), torch.tensor([-0.3])
    forms = [("num/den", num, den, None, float(num.double() / den.double())), ("num", num, None, None, float(num))]
    forms += [(f"lambda {lam}", None, None, lam, ref_softplus(lam)) for lam in LAMBDAS]
    for (what, nm, dn, lam, s), sign in ((f, sg) for f in forms for sg in (1.0, -1.0)):
        for av in ((a,) if lam is None else (a, torch.zeros(n))):
            ref = av.double() + sign * s * b.double()

            def body(alias):
                def run(k):
                    numd, dend, lamd = (None if nm is None else k.raw(nm)), (None if dn is None else k.raw(dn)), k.lam(lam)
                    if alias == "a":
                        o, bd = k.out((n,), av), k.inp(b)
                        ap, bp = o.ptr(), bd.data_ptr()
                    elif alias == "b":
                        ad, o = k.inp(av), k.out((n,), b)
                        ap, bp = ad.data_ptr(), o.ptr()
                    else:
                        ad, bd, o = k.inp(av), k.inp(b), k.out((n,))
                        ap, bp = ad.data_ptr(), bd.data_ptr()
                    check(L().cine_axpby_dev(o.ptr(), ap, bp, n, ptr(numd), ptr(dend), ptr(lamd), sign, stream()), "cine_axpby_dev")
                    return [o.t]
                return run
            got, = at_offsets(dev, OFFS, body(None), "cine_axpby_dev")
            _record(f"cine_axpby_dev ({what.split()[0]})", rel_err(got, ref), BAR, (n, what, sign))
            for alias in ("a", "b"):
                same, = twice(dev, 1, body(alias), f"cine_axpby_dev out == {alias}")
                assert same_bits(same, got), (n, what, sign, alias)


def _lam_factor(kind, lam):
    v = ref_softplus(lam)
    return (v, v / (1 + v), 1 / (1 + v) ** 2, 1 / (1 + v))[kind]


@gpu
@pytest.mark.parametrize("n", V_N)
def test_axpby_lam(dev, n):
    a, b = _rand(n * 3 + 1, n), _rand(n * 3 + 2, n)
    for kind in KINDS:
        for i, lam in enumerate(LAMBDAS):
            sign = (1.0, -1.0)[(i + kind) % 2]
            for av in (None, a):
                ref = sign * _lam_factor(kind, lam) * b.double() + (0 if av is None else av.double())

                def body(k):
                    ad, bd, lamd, o = k.inp(av), k.inp(b), k.lam(lam), k.out((n,))
                    check(L().cine_axpby_lam(o.ptr(), ptr(ad), bd.data_ptr(), n, lamd.data_ptr(), kind, sign, stream()), "cine_axpby_lam")
                    return [o.t]
                got, = at_offsets(dev, OFFS, body, "cine_axpby_lam")
                _record(f"cine_axpby_lam (kind {kind}, a {'NULL' if av is None else 'given'})", rel_err(got, ref), BAR, (n, lam, sign))


def _step_body(entry, n, x, r, p, d, rr_old, part32):
    """cine_cg_step / _pd / _pd2 on fresh operands: x, r, p in place, rr_new (and pd_out) pure outputs, the workspace exactly
    cine_cg_ws_bytes with the 256 p.d partials laid into its first 256 floats for the _pd forms."""
    def run(k):
        xg, rg, pg, dd, rro = k.out((n,), x), k.out((n,), r), k.out((n,), p), k.inp(d), k.raw(rr_old)
        rrn, ws = k.out((1,)), k.ws(L().cine_cg_ws_bytes())
        outs = [xg.t, rg.t, pg.t, rrn.t]
        if entry == "cine_cg_step":
            check(L().cine_cg_step(xg.ptr(), rg.ptr(), pg.ptr(), dd.data_ptr(), n, rro.data_ptr(), rrn.ptr(), ws.ptr(), stream()), entry)
            return outs
        ws.buf[:1024].view(torch.float32).copy_(part32)
        if entry == "cine_cg_step_pd":
            check(L().cine_cg_step_pd(xg.ptr(), rg.ptr(), pg.ptr(), dd.data_ptr(), n, rro.data_ptr(), rrn.ptr(), ws.ptr(), stream()), entry)
            return outs
        pdo = k.out((1,))
        check(L().cine_cg_step_pd2(xg.ptr(), rg.ptr(), pg.ptr(), dd.data_ptr(), n, rro.data_ptr(), rrn.ptr(), pdo.ptr(), ws.ptr(), stream()), entry)
        return outs + [pdo.t]
    return run


@gpu
@pytest.mark.parametrize("n", V_N)
def test_cg_step(dev, n):
    x, r, p, d, rr_old = cg_vectors(n)
    part32 = dot_partials(p, d).float()
    rn32 = ref_cg_step(x, r, p, d, rr_old[0])[3]             # torch's own float32 step: the yardstick above LONG_REDUCTION
    got_pd = None
    for entry in ("cine_cg_step", "cine_cg_step_pd", "cine_cg_step_pd2"):
        pd = None if entry == "cine_cg_step" else part32.double().sum()       # the _pd forms start from the partials they are given
        ref = ref_cg_step(x.double(), r.double(), p.double(), d.double(), rr_old.double()[0], pd)
        got = at_offsets(dev, OFFS, _step_body(entry, n, x, r, p, d, rr_old, part32), entry)
        for name, g, w in zip("xrp", got, ref):
            _record(f"{entry} ({name})", rel_err(g, w), BAR, n)
        _record(f"{entry} (rr_new)", _scalar_err(got[3], ref[3]), _bar(_scalar_err(rn32, ref[3]), n), n)
        if entry == "cine_cg_step_pd":
            got_pd = got
        if entry == "cine_cg_step_pd2":
            _record("cine_cg_step_pd2 (pd_out)", _scalar_err(got[4], ref[4]), BAR, n)
            for a, b in zip(got[:4], got_pd):
                assert same_bits(a, b), n                                     # cine_cg_step_pd2 is cine_cg_step_pd


@gpu
@pytest.mark.parametrize("n", V_N)
def test_cg_adjoint_step(dev, n):
    gp, q, gx, hg, pk, rr, pd, rr_new = adjoint_vectors(n)
    wgp, wq, ws = ref_adjoint_step(gp.double(), q.double(), gx.double(), hg.double(), pk.double(), rr.double()[0], pd.double()[0], rr_new.double()[0])
    scale = float((q.double() * pk.double()).abs().sum())

    def body(k):
        gpg, qg, gxd, hgd, pkd = k.out((n,), gp), k.out((n,), q), k.inp(gx), k.inp(hg), k.inp(pk)
        rrd, pdd, rnd_, part = k.raw(rr), k.raw(pd), k.raw(rr_new), k.out((256,))
        check(L().cine_cg_adjoint_step(gpg.ptr(), qg.ptr(), gxd.data_ptr(), hgd.data_ptr(), pkd.data_ptr(), n, rrd.data_ptr(), pdd.data_ptr(),
                                       rnd_.data_ptr(), part.ptr(), stream()), "cine_cg_adjoint_step")
        return [gpg.t, qg.t, part.t]
    ggp, gq, part = at_offsets(dev, OFFS, body, "cine_cg_adjoint_step")
    _record("cine_cg_adjoint_step (gp)", rel_err(ggp, wgp), BAR, n)
    _record("cine_cg_adjoint_step (q)", rel_err(gq, wq), BAR, n)
    _record("cine_cg_adjoint_step (<q, p_k>)", _scalar_err(part.double().sum(), ws, scale), _bar(_scalar_err(torch.dot(q, pk), ws, scale), n), n)
    assert rel_err(part, dot_partials(q, pk)) < BAR, n                       # each partial is its own workgroup's share


@gpu
@pytest.mark.parametrize("iters", FINISH_ITERS)
def test_cg_adjoint_finish(dev, iters):
    m = max(iters, 1)
    part = _rand(iters + 50, m * 256)
    rs = np.random.RandomState(iters + 60)
    rr, pd = (torch.from_numpy(rs.uniform(0.5, 2.0, n).astype(np.float32)) for n in (m + 1, m))
    sk = part.double().view(m, 256)
    al = rr.double()[:m] / pd.double()
    ref = -float((al * sk.sum(1))[:iters].sum())
    scale = float((al[:, None] * sk.abs())[:iters].sum())
    if iters == 0:                               # nothing may be read: every input NaN
        part, rr, pd = (torch.full_like(v, float("nan")) for v in (part, rr, pd))

    def body(k):
        pad, rrd, pdd, gv = k.inp(part), k.inp(rr), k.inp(pd), k.out((1,))
        check(L().cine_cg_adjoint_finish(pad.data_ptr(), rrd.data_ptr(), pdd.data_ptr(), iters, gv.ptr(), stream()), "cine_cg_adjoint_finish")
        return [gv.t]
    got, = at_offsets(dev, OFFS, body, "cine_cg_adjoint_finish")
    if iters == 0:
        assert float(got) == 0.0
    else:
        _record("cine_cg_adjoint_finish", _scalar_err(got, ref, scale), BAR, iters)


# ================================================================== F: one iteration with the operator inside
def _fused_body(kind, c, d, pd_out=True):
    b, t, C, w = c["b"], c["t"], c["c"], c["w"]
    lib = L()
    n = d["x"].numel()
    dc, cgf = lib.cine_image_dc_ws_bytes(b, t, C, H200, w), lib.cine_cg_fused_ws_bytes(b, t, C, H200, w)
    dims = (b, t, C, H200, w)

    def run(k):
        xg, rg, pg = k.out(d["x"].shape, d["x"]), k.out(d["r"].shape, d["r"]), k.out(d["p"].shape, d["p"])
        Sd, md, lamd, rro, rrn = k.inp(d["S"]), k.raw(d["mask"]), k.lam(c["lam"]), k.raw(d["rr_old"]), k.out((1,))
        wdc = k.ws(dc)
        if kind == "chain":                      # cine_normal_op_pd leaves the 256 partials where cine_cg_step_pd reads them
            dg, wcg = k.out(d["p"].shape), k.ws(lib.cine_cg_ws_bytes())
            check(lib.cine_normal_op_pd(pg.ptr(), Sd.data_ptr(), md.data_ptr(), lamd.data_ptr(), dg.ptr(), wcg.ptr(), *dims, wdc.ptr(), dc, stream()), "cine_normal_op_pd")
            check(lib.cine_cg_step_pd(xg.ptr(), rg.ptr(), pg.ptr(), dg.ptr(), n, rro.data_ptr(), rrn.ptr(), wcg.ptr(), stream()), "cine_cg_step_pd")
            return [xg.t, rg.t, pg.t, rrn.t]
        wcg = k.ws(cgf)
        pdo = k.out((1,)) if pd_out else None
        pdp = pdo.ptr() if pd_out else None
        if kind == "fused":
            check(lib.cine_normal_op_cg_fused(xg.ptr(), rg.ptr(), pg.ptr(), Sd.data_ptr(), md.data_ptr(), lamd.data_ptr(), rro.data_ptr(), rrn.ptr(), pdp,
                                              *dims, wdc.ptr(), dc, wcg.ptr(), cgf, stream()), "cine_normal_op_cg_fused")
        else:
            St = None
            if kind == "fused_t":
                St = k.out((lib.cine_sens_tile_floats(b, C, H200, w),))
                check(lib.cine_sens_tile_pack(Sd.data_ptr(), St.ptr(), b, C, H200, w, stream()), "cine_sens_tile_pack")
            check(lib.cine_normal_op_cg_fused_t(xg.ptr(), rg.ptr(), pg.ptr(), Sd.data_ptr(), None if St is None else St.ptr(), md.data_ptr(), lamd.data_ptr(),
                                                rro.data_ptr(), rrn.ptr(), pdp, *dims, wdc.ptr(), dc, wcg.ptr(), cgf, stream()), "cine_normal_op_cg_fused_t")
        return [xg.t, rg.t, pg.t, rrn.t] + ([pdo.t] if pd_out else [])
    return run


@gpu
@pytest.mark.parametrize("c", F_CASES, ids=case_id)
def test_cg_iteration_sweep(dev, c):
    d = f_ref(c)
    ref = d["ref"]
    assert float(ref[4]) > 0 and float(ref[3]) > 0
    got = {}
    for kind, entry in (("chain", "cine_normal_op_pd + cine_cg_step_pd"), ("fused", "cine_normal_op_cg_fused"), ("fused_t", "cine_normal_op_cg_fused_t"),
                        ("fused_t_null", "cine_normal_op_cg_fused_t")):
        got[kind] = g = twice(dev, 0, _fused_body(kind, c, d), entry)
        for name, a, w in zip("xrp", g, ref):
            _record(f"{entry} ({name})", rel_err(a.double().view(w.shape), w), BAR, case_id(c))
        _record(f"{entry} (rr_new)", _scalar_err(g[3], ref[3]), BAR, case_id(c))
        if kind != "chain":
            _record(f"{entry} (pd_out)", _scalar_err(g[4], ref[4]), BAR, case_id(c))
    for kind in ("fused_t", "fused_t_null"):                 # the tiled maps, or none, give the bits of the plain call
        for a, b in zip(got[kind], got["fused"]):
            assert same_bits(a, b), (c, kind)
    nopd = twice(dev, 0, _fused_body("fused", c, d, pd_out=False), "cine_normal_op_cg_fused pd_out=NULL")
    for a, b in zip(nopd, got["fused"]):
        assert same_bits(a, b), c


# ================================================================== S: the whole solve
def _solve_body(entry, c, d, tiled, past256=None, iters=None):
    b, t, C, w = c["b"], c["t"], c["c"], c["w"]
    iters = c["iters"] if iters is None else iters
    lib = L()
    nbytes = lib.cine_conj_grad_ws_bytes(b, t, C, H200, w)
    dims = (b, t, C, H200, w)

    def run(k):
        xg, rhs, Sd, md, lamd = k.out(d["x0"].shape, d["x0"]), k.inp(d["rhs"]), k.inp(d["S"]), k.raw(d["mask"]), k.lam(c["lam"])
        St = None
        if tiled:
            St = k.out((lib.cine_sens_tile_floats(b, C, H200, w),))
            check(lib.cine_sens_tile_pack(Sd.data_ptr(), St.ptr(), b, C, H200, w, stream()), "cine_sens_tile_pack")
        ws = k.ws(nbytes, past256)
        stp = None if St is None else St.ptr()
        if entry == "cine_conj_grad":
            check(lib.cine_conj_grad(xg.ptr(), rhs.data_ptr(), c["rhs_is_ref"], Sd.data_ptr(), stp, md.data_ptr(), lamd.data_ptr(), iters, *dims,
                                     ws.ptr(), nbytes, stream()), entry)
            return [xg.t]
        prec, rrrec, pdrec = k.out((iters,) + tuple(d["x0"].shape)), k.out((iters + 1,)), k.out((iters,))
        check(lib.cine_conj_grad_rec(xg.ptr(), rhs.data_ptr(), c["rhs_is_ref"], Sd.data_ptr(), stp, md.data_ptr(), lamd.data_ptr(), iters, *dims,
                                     ws.ptr(), nbytes, prec.ptr(), rrrec.ptr(), pdrec.ptr(), stream()), entry)
        return [xg.t, prec.t, rrrec.t, pdrec.t]
    return run


@gpu
@pytest.mark.parametrize("c", S_CASES, ids=case_id)
def test_conj_grad_sweep(dev, c):
    d = s_ref(c)
    x64, P64, RR64, PD64 = d["ref"]
    e32, iters = d["e32"], c["iters"]
    x, prec, rrrec, pdrec = twice(dev, 0, _solve_body("cine_conj_grad_rec", c, d, False), "cine_conj_grad_rec")
    for k in range(iters):
        _record("cine_conj_grad_rec (p_k)", rel_err(prec[k], pairs(P64[k])), chained_bar(e32["p"][k]), (case_id(c), k))
        _record("cine_conj_grad_rec (pd_k)", _scalar_err(pdrec[k], PD64[k]), chained_bar(e32["pd"][k]), (case_id(c), k))
    for k in range(iters + 1):
        _record("cine_conj_grad_rec (rr_k)", _scalar_err(rrrec[k], RR64[k]), chained_bar(e32["rr"][k]), (case_id(c), k))
    _record("cine_conj_grad_rec (x)", rel_err(x, pairs(x64)), chained_bar(e32["x"]), case_id(c))
    # the identities on the device's own records, in float64: no conditioning enters
    S, mask = cplx(d["S"]), d["mask"]
    acc = d["x0"].double()
    for k in range(iters):
        acc = acc + (rrrec[k].double() / pdrec[k].double()) * prec[k].double()
        pk = cplx(prec[k])
        _record("cine_conj_grad_rec (pd_k = <p_k, H p_k>)", _scalar_err(pdrec[k], rdot(pk, ref_normal_op(pk, S, mask, c["lam"]))), BAR, (case_id(c), k))
    _record("cine_conj_grad_rec (x = x0 + sum alpha_k p_k)", rel_err(x, acc), BAR, case_id(c))
    # the tiled maps give the same bits, and cine_conj_grad the bits of cine_conj_grad_rec's x
    for a, b in zip(twice(dev, 0, _solve_body("cine_conj_grad_rec", c, d, True), "cine_conj_grad_rec (tiled)"), (x, prec, rrrec, pdrec)):
        assert same_bits(a, b), c
    for tiled in (False, True):
        xs, = twice(dev, 0, _solve_body("cine_conj_grad", c, d, tiled), "cine_conj_grad")
        assert same_bits(xs, x), (c, tiled)
    _record("cine_conj_grad (x)", rel_err(xs, pairs(x64)), chained_bar(e32["x"]), case_id(c))


@gpu
def test_conj_grad_workspace_16_bytes_past_a_256_byte_boundary(dev):
    """The solver rounds the {p, r} pairs inside its workspace up to 256 bytes; cine_conj_grad_ws_bytes pays for that with its + 256.  A
    base 16 bytes past a boundary and exactly that many bytes: the tail stays intact and the bits are those of the aligned call."""
    c = WS_CASE
    d = s_ref(c)
    want, = twice(dev, 0, _solve_body("cine_conj_grad", c, d, False), "cine_conj_grad")
    got, = twice(dev, 0, _solve_body("cine_conj_grad", c, d, False, past256=16), "cine_conj_grad (workspace 16 bytes past a 256-byte boundary)")
    assert same_bits(got, want)
    _record("cine_conj_grad (x)", rel_err(got, pairs(d["ref"][0])), chained_bar(d["e32"]["x"]), case_id(c))
    rec = twice(dev, 0, _solve_body("cine_conj_grad_rec", c, d, True, past256=16), "cine_conj_grad_rec (workspace 16 bytes past a 256-byte boundary)")
    assert same_bits(rec[0], want)


@gpu
@pytest.mark.parametrize("c", IDENTITY_CASES, ids=case_id)
def test_conj_grad_one_exact_step_on_a_multiple_of_the_identity(dev, c):
    """Masks "all" and "none" with normalised maps: H = (1 + v) I or v I up to the rounding of the maps, so one iteration solves the system.
    Everything in front of the step is a single evaluation from the inputs and meets BAR (x, p_0, rr_0, pd_0).  rr_1 is zero in exact
    arithmetic: the residual it sums must lie within BAR of the first one, sqrt(rr_1 / rr_0) <= BAR."""
    d = s_ref(c)
    x64, P64, RR64, PD64 = d["ref"]
    x, prec, rrrec, pdrec = twice(dev, 0, _solve_body("cine_conj_grad_rec", c, d, False), "cine_conj_grad_rec")
    _record("cine_conj_grad_rec (x, exact step)", rel_err(x, pairs(x64)), BAR, case_id(c))
    _record("cine_conj_grad_rec (p_0, exact step)", rel_err(prec[0], pairs(P64[0])), BAR, case_id(c))
    _record("cine_conj_grad_rec (rr_0, exact step)", _scalar_err(rrrec[0], RR64[0]), BAR, case_id(c))
    _record("cine_conj_grad_rec (pd_0, exact step)", _scalar_err(pdrec[0], PD64[0]), BAR, case_id(c))
    assert float(rrrec[1]) >= 0
    _record("cine_conj_grad_rec (sqrt(rr_1 / rr_0), exact step)", float(rrrec[1].double() / rrrec[0].double()) ** 0.5, BAR, case_id(c))
    for tiled in (False, True):
        xs, = twice(dev, 0, _solve_body("cine_conj_grad", c, d, tiled), "cine_conj_grad")
        assert same_bits(xs, x), (c, tiled)


@gpu
@pytest.mark.parametrize("c", ZERO_ITERS_CASES, ids=case_id)
def test_conj_grad_without_an_iteration_returns_its_start_value(dev, c):
    d = s_ref(c)
    for tiled in (False, True):
        x, = twice(dev, 0, _solve_body("cine_conj_grad", c, d, tiled), "cine_conj_grad iters=0")
        assert same_bits(x, d["x0"]), c


# ================================================================== refusals: decided on the host, before any launch
@gpu
def test_vector_refusals(dev):
    lib, st, n = L(), stream(), 5
    x, r, p, d, rr_old = cg_vectors(n)
    k = Call(dev, 0)
    xg, rg, pg, dd, rro, rrn, pdo = k.out((n,), x), k.out((n,), r), k.out((n,), p), k.inp(d), k.raw(rr_old), k.out((1,)), k.out((1,))
    ws, part, o = k.ws(lib.cine_cg_ws_bytes()), k.out((256,)), k.out((n,))
    X, R, P_, D, RO, RN, PO, W = xg.ptr(), rg.ptr(), pg.ptr(), dd.data_ptr(), rro.data_ptr(), rrn.ptr(), pdo.ptr(), ws.ptr()

    def swap(args, i, v):
        return args[:i] + (v,) + args[i + 1:]
    for name, args, nulls in (("cine_cg_step", (X, R, P_, D, n, RO, RN, W, st), (0, 1, 2, 3, 5, 6, 7)),
                              ("cine_cg_step_pd", (X, R, P_, D, n, RO, RN, W, st), (0, 1, 2, 3, 5, 6, 7)),
                              ("cine_cg_step_pd2", (X, R, P_, D, n, RO, RN, PO, W, st), (0, 1, 2, 3, 5, 6, 7, 8)),
                              ("cine_dot", (D, D, n, RN, W, st), (0, 1, 3, 4)),
                              ("cine_axpby_dev", (o.ptr(), D, D, n, RO, None, None, 1.0, st), (0, 1, 2)),
                              ("cine_axpby_lam", (o.ptr(), D, D, n, RO, 0, 1.0, st), (0, 2, 4)),
                              ("cine_cg_adjoint_step", (X, R, D, D, D, n, RO, RO, RO, part.ptr(), st), (0, 1, 2, 3, 4, 6, 7, 8, 9)),
                              ("cine_cg_adjoint_finish", (part.ptr(), RO, RO, 1, RN, st), (0, 1, 2, 4))):
        entry = getattr(lib, name)
        for i in nulls:
            refused(lambda: entry(*swap(args, i, None)), EINVAL, k, f"{name} argument {i} NULL")
        if name != "cine_cg_adjoint_finish":
            ni = args.index(n)
            for bad in (0, -1):
                refused(lambda: entry(*swap(args, ni, bad)), EINVAL, k, f"{name} n={bad}")
        if name.startswith("cine_cg_step"):
            refused(lambda: entry(*swap(args, 6, RO)), EINVAL, k, f"{name} rr_old == rr_new")
    refused(lambda: lib.cine_axpby_dev(o.ptr(), D, D, n, None, None, None, 1.0, st), EINVAL, k, "cine_axpby_dev neither num nor lambda")
    for kind in (-1, 4):
        refused(lambda: lib.cine_axpby_lam(o.ptr(), D, D, n, RO, kind, 1.0, st), EINVAL, k, f"cine_axpby_lam kind={kind}")
    refused(lambda: lib.cine_cg_adjoint_finish(part.ptr(), RO, RO, -1, RN, st), EINVAL, k, "cine_cg_adjoint_finish iters=-1")


def _solver_operands(dev, b, t, C, h, w, iters=2, zeros=False):
    """Every operand of the F and S entry points at its full size, and the calls with one argument replaced."""
    lib, st = L(), stream()
    k = Call(dev, 0)
    mk = (lambda s, *shape: torch.zeros(*shape)) if zeros else _rand
    xg, rg, pg = (k.out((b, t, h, w, 2), mk(i, b, t, h, w, 2)) for i in (1, 2, 3))
    Sd, md, lamd, rro = k.inp(mk(4, b, C, h, w, 2)), k.raw(torch.ones(b, t, h, dtype=torch.uint8)), k.lam(0.5), k.raw(torch.tensor([1.5]))
    rrn, pdo, prec, rrrec, pdrec = k.out((1,)), k.out((1,)), k.out((iters, b, t, h, w, 2)), k.out((iters + 1,)), k.out((iters,))
    sizes = dict(dc=lib.cine_image_dc_ws_bytes(b, t, C, h, w), cgf=lib.cine_cg_fused_ws_bytes(b, t, C, h, w), cg=lib.cine_conj_grad_ws_bytes(b, t, C, h, w))
    # where the shape has no workspace size the calls still get real buffers: a refusal must come before anything is touched
    wdc, wcg, wcj = k.ws(sizes["dc"] or 64), k.ws(sizes["cgf"] or 64), k.ws(sizes["cg"] or 64)
    a = dict(x=xg.ptr(), r=rg.ptr(), p=pg.ptr(), rhs=rg.ptr(), sens=Sd.data_ptr(), mask=md.data_ptr(), lam=lamd.data_ptr(), rr_old=rro.data_ptr(), rr_new=rrn.ptr(),
             pd_out=pdo.ptr(), b=b, t=t, c=C, h=h, w=w, ws_dc=wdc.ptr(), ws_dc_bytes=sizes["dc"], ws_cg=wcg.ptr(), ws_cg_bytes=sizes["cgf"], ws=wcj.ptr(),
             ws_bytes=sizes["cg"], iters=iters, rhs_is_ref=0, p_rec=prec.ptr(), rr_rec=rrrec.ptr(), pd_rec=pdrec.ptr(), tiled=None)

    def fused(**kw):
        v = dict(a, **kw)
        return lib.cine_normal_op_cg_fused(v["x"], v["r"], v["p"], v["sens"], v["mask"], v["lam"], v["rr_old"], v["rr_new"], v["pd_out"], v["b"], v["t"], v["c"], v["h"],
                                           v["w"], v["ws_dc"], v["ws_dc_bytes"], v["ws_cg"], v["ws_cg_bytes"], st)

    def fused_t(**kw):
        v = dict(a, **kw)
        return lib.cine_normal_op_cg_fused_t(v["x"], v["r"], v["p"], v["sens"], v["tiled"], v["mask"], v["lam"], v["rr_old"], v["rr_new"], v["pd_out"], v["b"], v["t"],
                                             v["c"], v["h"], v["w"], v["ws_dc"], v["ws_dc_bytes"], v["ws_cg"], v["ws_cg_bytes"], st)

    def solve(**kw):
        v = dict(a, **kw)
        return lib.cine_conj_grad(v["x"], v["rhs"], v["rhs_is_ref"], v["sens"], v["tiled"], v["mask"], v["lam"], v["iters"], v["b"], v["t"], v["c"], v["h"], v["w"],
                                  v["ws"], v["ws_bytes"], st)

    def solve_rec(**kw):
        v = dict(a, **kw)
        return lib.cine_conj_grad_rec(v["x"], v["rhs"], v["rhs_is_ref"], v["sens"], v["tiled"], v["mask"], v["lam"], v["iters"], v["b"], v["t"], v["c"], v["h"], v["w"],
                                      v["ws"], v["ws_bytes"], v["p_rec"], v["rr_rec"], v["pd_rec"], st)
    return k, a, sizes, fused, fused_t, solve, solve_rec


FUSED_NAME, SOLVE_NAME = "cine_normal_op_cg_fused", "cine_conj_grad"           # the messages of the _t / _rec forms name the common body


@gpu
def test_solver_refusals(dev):
    k, a, sizes, fused, fused_t, solve, solve_rec = _solver_operands(dev, 2, 2, 7, H200, 3)
    assert all(v > 0 for v in sizes.values())
    for arg in ("x", "r", "p", "sens", "mask", "lam", "rr_old", "rr_new", "ws_dc", "ws_cg"):
        for call, what in ((fused, "cine_normal_op_cg_fused"), (fused_t, "cine_normal_op_cg_fused_t")):
            refused(lambda: call(**{arg: None}), EINVAL, k, f"{what} {arg}=NULL", FUSED_NAME)
    for call, what in ((fused, "cine_normal_op_cg_fused"), (fused_t, "cine_normal_op_cg_fused_t")):
        refused(lambda: call(rr_new=a["rr_old"]), EINVAL, k, f"{what} rr_old == rr_new", FUSED_NAME)
        refused(lambda: call(ws_cg_bytes=sizes["cgf"] - 1), EWORKSPACE, k, f"{what} ws_cg one byte short", FUSED_NAME)
        refused(lambda: call(ws_dc_bytes=sizes["dc"] - 1), EWORKSPACE, k, f"{what} ws_dc one byte short", FUSED_NAME)
    for call, what in ((solve, "cine_conj_grad"), (solve_rec, "cine_conj_grad_rec")):
        for arg in ("x", "rhs", "sens", "mask", "lam", "ws"):
            refused(lambda: call(**{arg: None}), EINVAL, k, f"{what} {arg}=NULL", SOLVE_NAME)
        refused(lambda: call(rhs=a["x"]), EINVAL, k, f"{what} x == rhs", SOLVE_NAME)
        refused(lambda: call(iters=-1), EINVAL, k, f"{what} iters=-1", SOLVE_NAME)
        refused(lambda: call(ws_bytes=sizes["cg"] - 1), EWORKSPACE, k, f"{what} workspace one byte short", SOLVE_NAME)
    refused(lambda: solve_rec(iters=0), EINVAL, k, "cine_conj_grad_rec iters=0")
    for arg in ("p_rec", "rr_rec", "pd_rec"):
        refused(lambda: solve_rec(**{arg: None}), EINVAL, k, f"cine_conj_grad_rec {arg}=NULL")


@gpu
@pytest.mark.parametrize("C,h", [(7, 24), (5, 200), (1, 200), (7, 199)])
def test_solver_refuses_shapes_without_the_200_row_coil_group_kernel(dev, C, h):
    lib = L()
    b, t, w = 1, 2, 3
    assert lib.cine_cg_fused_ws_bytes(b, t, C, h, w) == 0 and lib.cine_conj_grad_ws_bytes(b, t, C, h, w) == 0
    assert lib.cine_image_dc_ws_bytes(b, t, C, h, w) == 0
    k, a, sizes, fused, fused_t, solve, solve_rec = _solver_operands(dev, b, t, C, h, w)
    big = 1 << 20                                # no size can make the shape supported
    refused(lambda: fused(ws_dc_bytes=big, ws_cg_bytes=big), EUNSUPPORTED, k, "cine_normal_op_cg_fused", FUSED_NAME)
    refused(lambda: fused_t(ws_dc_bytes=big, ws_cg_bytes=big), EUNSUPPORTED, k, "cine_normal_op_cg_fused_t", FUSED_NAME)
    refused(lambda: solve(ws_bytes=big), EUNSUPPORTED, k, "cine_conj_grad", SOLVE_NAME)
    refused(lambda: solve_rec(ws_bytes=big), EUNSUPPORTED, k, "cine_conj_grad_rec", SOLVE_NAME)


@gpu
def test_solver_refuses_more_than_65535_frames(dev):
    """b * t = 65 536 frames of one column: every buffer has its full size."""
    k, a, sizes, fused, fused_t, solve, solve_rec = _solver_operands(dev, 2, 32768, 6, H200, 1, iters=1, zeros=True)
    assert all(v > 0 for v in sizes.values())
    refused(lambda: fused(), EUNSUPPORTED, k, "cine_normal_op_cg_fused b*t=65536")
    refused(lambda: fused_t(), EUNSUPPORTED, k, "cine_normal_op_cg_fused_t b*t=65536", FUSED_NAME)
    refused(lambda: solve(), EUNSUPPORTED, k, "cine_conj_grad b*t=65536")
    refused(lambda: solve_rec(), EUNSUPPORTED, k, "cine_conj_grad_rec b*t=65536", SOLVE_NAME)
