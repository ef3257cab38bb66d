"""cine_hip.augment on the host: the convention of cine_affine_warp (tests/augment_reference.py, float64 numpy) against
torch.nn.functional.grid_sample in float64, the matrices of from_params / compose, the frame remap, sample, schedule, and every
validation error by the field it names.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_reference as R
from cine_hip import augment as A
from cine_hip._lib import CineHipError, parse_header, HEADER_PATH

SHAPES = [(1, 1), (1, 4), (2, 3), (5, 8), (17, 33), (20, 12)]
IDENT = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0))


def grid_sample_f64(x, m, mode, border):
    """x (planes, h, w, 2) float64 -> the same through affine_grid + grid_sample(align_corners=False) in float64."""
    p, h, w, _ = x.shape
    n = torch.from_numpy(x).permute(0, 3, 1, 2).reshape(1, 2 * p, h, w)
    grid = F.affine_grid(torch.from_numpy(R.theta_of(m, h, w))[None], (1, 2 * p, h, w), align_corners=False)
    y = F.grid_sample(n, grid, mode=("bilinear", "bicubic")[mode], padding_mode=("zeros", "reflection")[border], align_corners=False)
    return y.reshape(p, 2, h, w).permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_against_grid_sample(hw):
    h, w = hw
    x = np.random.RandomState(7 * h + w).standard_normal((3, h, w, 2))
    worst = 0.0
    for name, m in R.matrices(h, w).items():
        for mode in (0, 1):
            for border in (0, 1):
                got, _ = R.warp_planes(x, m, mode, border)
                err = float(np.abs(got - grid_sample_f64(x, m, mode, border)).max())
                worst = max(worst, err)
                assert err <= 1e-11, f"{h}x{w} {name} mode {mode} border {border}: {err:.3e}"
    print(f"{h}x{w}: worst |restatement - grid_sample| {worst:.2e}")


def test_restatement_exact_cases():
    x = np.random.RandomState(3).standard_normal((2, 6, 6, 2))
    ms = R.matrices(6, 6)
    for mode in (0, 1):
        for border in (0, 1):
            assert np.array_equal(R.warp_planes(x, ms["identity"], mode, border)[0], x)
            assert np.array_equal(R.warp_planes(x, ms["flip_h"], mode, border)[0], x[:, :, ::-1])
            assert np.array_equal(R.warp_planes(x, ms["flip_v"], mode, border)[0], x[:, ::-1])
            assert np.array_equal(R.warp_planes(x, ms["rot90"], mode, border)[0], np.rot90(x, 1, (1, 2)))
    assert list(R.reflect(np.arange(-7, 8), 3)) == [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1]
    assert list(R.reflect(np.arange(-3, 4), 1)) == [0] * 7


def test_header_declares_the_entry_point():
    import ctypes
    sigs = parse_header(open(HEADER_PATH).read())
    res, args = sigs["cine_affine_warp"]
    assert res is ctypes.c_int and len(args) == 17
    assert args[:2] == [ctypes.c_void_p] * 2 and args[2:6] == [ctypes.c_int] * 4 and args[6:12] == [ctypes.c_double] * 6
    assert args[12:16] == [ctypes.c_int] * 4 and args[16] is ctypes.c_void_p


# ---------------------------------------------------------------------- from_params / compose
def test_from_params_integral_cases():
    for h, w in ((8, 8), (7, 7), (5, 9)):
        cases = [dict(flip_h=True), dict(flip_v=True), dict(flip_h=True, flip_v=True), dict(translate=(3, -2)),
                 dict(flip_h=True, translate=(-1, 4))]
        if h == w:
            cases += [dict(rot90=k) for k in (1, 2, 3, 5, -1)] + [dict(rot90=1, flip_v=True, translate=(2, 1))]
        for kw in cases:
            m = A.Augmentation.from_params(h, w, **kw).array()
            assert np.array_equal(m, np.round(m)), (kw, m)
            assert not np.signbit(m).any() or (m[np.signbit(m)] != 0).all(), "a negative zero"
    assert A.Augmentation.from_params(6, 4).matrix == IDENT
    assert A.Augmentation.from_params(6, 4) == A.identity()
    assert A.Augmentation.from_params(8, 8, flip_h=True).matrix == ((1.0, 0.0, 0.0), (0.0, -1.0, 0.0))
    assert A.Augmentation.from_params(8, 8, rot90=1).matrix == R.matrices(8, 8)["rot90"]
    assert A.Augmentation.from_params(8, 8, translate=(3, -2)).matrix == ((1.0, 0.0, -3.0), (0.0, 1.0, 2.0))


def test_from_params_matches_the_array_operations():
    """The map of flips / quarter turns / integer shifts, applied by the float64 restatement, is the array operation."""
    x = np.random.RandomState(5).standard_normal((1, 6, 6, 2))
    for k in range(4):
        m = A.Augmentation.from_params(6, 6, rot90=k).matrix
        assert np.array_equal(R.warp_planes(x, m, 1, 1)[0], np.rot90(x, k, (1, 2)))
    m = A.Augmentation.from_params(6, 6, flip_h=True, rot90=1).matrix                  # the flip first, then the quarter turn
    assert np.array_equal(R.warp_planes(x, m, 0, 0)[0], np.rot90(x[:, :, ::-1], 1, (1, 2)))
    m = A.Augmentation.from_params(6, 6, translate=(2, -1)).matrix                     # the content moves by (+2, -1)
    pad = np.pad(x, ((0, 0), (6, 6), (6, 6), (0, 0)), mode="symmetric")
    assert np.array_equal(R.warp_planes(x, m, 1, 1)[0], pad[:, 6 - 2:12 - 2, 6 + 1:12 + 1])
    rot = A.Augmentation.from_params(6, 6, rotation_deg=90.0).array()                  # a rotation by 90 degrees is a quarter turn, nearly
    assert np.abs(rot - np.array(R.matrices(6, 6)["rot90"])).max() < 1e-15


def test_inverse_times_forward_is_identity():
    rs = np.random.RandomState(11)
    for _ in range(50):
        h, w = (int(rs.randint(1, 300)),) * 2 if rs.rand() < 0.5 else (int(rs.randint(1, 300)), int(rs.randint(1, 300)))
        kw = dict(rotation_deg=float(rs.uniform(-180, 180)), scale=tuple(rs.uniform(0.5, 2.0, 2)), shear_deg=tuple(rs.uniform(-30, 30, 2)),
                  translate=tuple(rs.uniform(-40, 40, 2)), flip_h=bool(rs.randint(2)), flip_v=bool(rs.randint(2)),
                  rot90=int(rs.randint(4)) if h == w else 0)
        fwd, inv = A.affine_matrices(h, w, **kw)
        scale = max(1.0, np.abs(fwd).max() * np.abs(inv).max())
        assert np.abs(fwd @ inv - np.eye(3)).max() <= 1e-12 * scale and np.abs(inv @ fwd - np.eye(3)).max() <= 1e-12 * scale, kw
        assert np.array_equal(np.array(A.Augmentation.from_params(h, w, **kw).matrix), inv[:2])


def test_compose():
    rs = np.random.RandomState(13)
    mk = lambda: A.Augmentation.from_params(32, 32, rotation_deg=float(rs.uniform(-90, 90)), scale=tuple(rs.uniform(0.7, 1.4, 2)),
                                            translate=tuple(rs.uniform(-5, 5, 2)), flip_h=bool(rs.randint(2)), rot90=int(rs.randint(4)),
                                            t_shift=int(rs.randint(0, 7)), t_reverse=bool(rs.randint(2)))
    for _ in range(20):
        a, b, c = mk(), mk(), mk()
        left, right = A.compose(A.compose(a, b), c), A.compose(a, A.compose(b, c))
        assert np.abs(left.array() - right.array()).max() <= 1e-12 * max(1.0, np.abs(left.array()).max())
        assert left.t_reverse == right.t_reverse
        for frames in (1, 2, 5, 7):
            assert np.array_equal(left.frame_map(frames), right.frame_map(frames))
            assert np.array_equal(A.compose(a, b).frame_map(frames), a.frame_map(frames)[b.frame_map(frames)])    # a first, then b
        assert np.array_equal(A.compose(a, b).homogeneous(), a.homogeneous() @ b.homogeneous() + 0.0)
        assert A.compose(a, A.identity()).matrix == a.matrix and A.compose(A.identity(), a).matrix == a.matrix
    a = A.Augmentation.from_params(8, 8, flip_h=True, mode="bilinear", border="zeros")
    assert (A.compose(a, A.identity()).mode, A.compose(a, A.identity()).border) == ("bilinear", "zeros")
    assert A.compose(a, a, mode="bicubic", border="reflect") == A.identity()
    with pytest.raises(CineHipError, match="two Augmentation"):
        A.compose(a, IDENT)


# ---------------------------------------------------------------------- the frame remap
@pytest.mark.parametrize("frames", [1, 2, 5])
def test_frame_map_is_a_permutation(frames):
    x = np.arange(frames)
    for s in range(-frames, 2 * frames + 1):
        for rev in (False, True):
            g = A.Augmentation(t_shift=s, t_reverse=rev).frame_map(frames)
            assert sorted(g) == list(range(frames)), (s, rev, g)
            assert np.array_equal(g, R.frame_map(frames, s % frames, rev))               # the kernel gets the shift reduced
            want = np.roll(x[::-1], s + 1) if rev else np.roll(x, -s)
            assert np.array_equal(x[g], want), (s, rev)
            for f in range(frames):                                                      # the mathematical mod, spelled out
                src = (s - f) if rev else (f + s)
                while src < 0:
                    src += frames
                assert g[f] == src % frames
    rs = np.random.RandomState(frames).standard_normal((frames, 2, 3, 4, 2))
    out, _ = R.warp_reference(rs, IDENT, 1, 1, t_shift=frames - 1, t_reverse=True)
    assert np.array_equal(out, rs[R.frame_map(frames, frames - 1, True)])


# ---------------------------------------------------------------------- sample / schedule
def test_sample_is_repeatable_per_example():
    a = A.sample((3, 2, 17), 200, 200, p=0.9, frames=15)
    assert a == A.sample((3, 2, 17), 200, 200, p=0.9, frames=15) == A.sample([3, 2, 17], 200, 200, p=0.9, frames=15)
    assert a == A.sample(np.random.default_rng([3, 2, 17]), 200, 200, p=0.9, frames=15)
    others = [A.sample(k, 200, 200, p=0.9, frames=15) for k in ((4, 2, 17), (3, 3, 17), (3, 2, 18))]
    assert all(o != a for o in others) and len({o.matrix for o in others}) == 3
    for k in range(30):
        assert A.sample((1, 0, k), 64, 48, p=0.0, frames=9) == A.identity()
        full = A.sample((1, 0, k), 64, 48, p=1.0, frames=9, weight_flip_h=1.0, weight_flip_v=1.0, weight_t_shift=1.0, weight_t_reverse=1.0)
        assert 0 <= full.t_shift < 9 and full.t_reverse and full.matrix != IDENT
        assert A.sample((1, 0, k), 64, 48, p=1.0).t_shift == 0 and not A.sample((1, 0, k), 64, 48, p=1.0).t_reverse    # no frames: no temporal part
    assert A.sample(5, 64, 64, p=0.7) == A.sample([5], 64, 64, p=0.7)
    assert A.sample(5, 64, 64, p=1.0, mode="bilinear", border="zeros").mode == "bilinear"


def test_sample_ranges_and_rates():
    n = 400
    draws = [A.sample((9, 0, k), 100, 80, p=0.5, frames=12, rotation=0.0, shear=0.0, scale=0.0, weight_rot90=0.0) for k in range(n)]
    # only translations, flips and the temporal part remain: the linear part is a diagonal of +-1
    for d in draws:
        m = d.array()
        assert abs(m[0, 0]) == 1.0 and abs(m[1, 1]) == 1.0 and m[0, 1] == 0.0 and m[1, 0] == 0.0
        assert abs(m[0, 2]) <= 0.08 * 100 and abs(m[1, 2]) <= 0.125 * 80
    rate = lambda pred: sum(map(pred, draws)) / n
    assert abs(rate(lambda d: d.matrix[1][1] < 0) - 0.25) < 0.08                         # flip_h: p * 0.5
    assert abs(rate(lambda d: d.t_reverse) - 0.25) < 0.08
    assert abs(rate(lambda d: d.matrix[0][2] != 0.0) - 0.5) < 0.08                       # translation: p * 1
    only_rot = A.sample((2, 2, 2), 64, 64, p=1.0, shear=0.0, scale=0.0, translate=(0.0, 0.0), weight_flip_h=0, weight_flip_v=0, weight_rot90=0)
    m = only_rot.array()[:, :2]
    assert np.abs(m @ m.T - np.eye(2)).max() < 1e-12 and abs(np.linalg.det(m) - 1.0) < 1e-12


def test_schedule():
    assert A.schedule(0, 50) == 0.0
    assert A.schedule(50, 50) == pytest.approx(0.55, abs=1e-15)
    assert A.schedule(20, 20, p_max=0.3, decay=2.0) == pytest.approx(0.3, abs=1e-15)
    p = [A.schedule(e, 50) for e in range(51)]
    assert all(b > a for a, b in zip(p, p[1:])) and all(0.0 <= v <= 0.55 for v in p)
    assert A.schedule(25, 50) == pytest.approx(0.55 * (1 - np.exp(-2.5)) / (1 - np.exp(-5.0)), rel=1e-14)
    for bad in (dict(epoch=-1, epochs=10), dict(epoch=11, epochs=10), dict(epoch=0, epochs=0), dict(epoch=1, epochs=10, p_max=1.5),
                dict(epoch=1, epochs=10, decay=0.0)):
        with pytest.raises(CineHipError, match="schedule"):
            A.schedule(**bad)


# ---------------------------------------------------------------------- validation, by field
def test_validation_names_the_field():
    ok = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    bad = [
        ("matrix", dict(matrix=((1.0, 0.0), (0.0, 1.0)))),
        ("matrix", dict(matrix="abc")),
        ("matrix", dict(matrix=((1.0, 0.0, float("nan")), (0.0, 1.0, 0.0)))),
        ("matrix", dict(matrix=((float("inf"), 0.0, 0.0), (0.0, 1.0, 0.0)))),
        ("matrix", dict(matrix=((1.0, 0.0, 0.0), (0.0, -1024.5, 0.0)))),
        ("matrix", dict(matrix=((1.0, 0.0, 0.0), (0.0, 1.0, 2.0 ** 20 + 1)))),
        ("t_shift", dict(t_shift=1.5)),
        ("t_shift", dict(t_shift=True)),
        ("t_reverse", dict(t_reverse=1)),
        ("mode", dict(mode="nearest")),
        ("mode", dict(mode=1)),
        ("border", dict(border="wrap")),
    ]
    for field, kw in bad:
        with pytest.raises(CineHipError, match=rf"Augmentation: {field}:"):
            A.Augmentation(**{"matrix": ok, **kw})
    A.Augmentation(((1024.0, -1024.0, 2.0 ** 20), (0.0, 0.0, -2.0 ** 20)))                # the limits themselves pass
    a = A.identity()
    with pytest.raises(Exception):                                                        # immutable
        a.t_shift = 3
    bad_params = [
        ("h, w", dict(h=0)), ("h, w", dict(w=4097)), ("h, w", dict(h=2.0)),
        ("rot90", dict(h=8, w=6, rot90=1)), ("rot90", dict(rot90=0.5)),
        ("rotation_deg", dict(rotation_deg=float("nan"))), ("rotation_deg", dict(rotation_deg="a")),
        ("scale", dict(scale=(1.0, 0.0))), ("scale", dict(scale=(1.0, 2.0, 3.0))), ("scale", dict(scale=float("inf"))),
        ("shear_deg", dict(shear_deg=(45.0, 45.0))), ("shear_deg", dict(shear_deg=(90.0, 0.0))),
        ("translate", dict(translate=(float("nan"), 0.0))), ("translate", dict(translate="x")),
        ("matrix", dict(translate=(2.0 ** 21, 0.0))), ("matrix", dict(scale=(1e-4, 1.0))),
        ("mode", dict(mode="cubic")), ("border", dict(border="reflection")), ("t_shift", dict(t_shift=0.5)),
    ]
    for field, kw in bad_params:
        args = {"h": 8, "w": 8, **kw}
        with pytest.raises(CineHipError, match=rf": {field}:"):
            A.Augmentation.from_params(**args)
    assert A.Augmentation.from_params(8, 6, rot90=4).matrix == IDENT                      # whole turns need no square
    for field, call in [("p", lambda: A.sample(1, 8, 8, p=1.5)), ("frames", lambda: A.sample(1, 8, 8, frames=0)),
                        ("rng_or_seed", lambda: A.sample("seed", 8, 8)), ("rng_or_seed", lambda: A.sample((1, -2), 8, 8)),
                        ("translate", lambda: A.sample(1, 8, 8, translate=(1, 2, 3)))]:
        with pytest.raises(CineHipError, match=rf": {field}:"):
            call()


def test_prepare_example_has_the_front_ends_arguments_and_augment_last():
    import inspect
    from cine_hip import frontend as FE
    fe, au = inspect.signature(FE.prepare_example).parameters, inspect.signature(A.prepare_example).parameters
    assert list(au) == list(fe) + ["augment"] and au["augment"].default is None
    assert all(au[k].default == fe[k].default for k in fe)
    assert list(fe)[-1] == "whitener"                                                     # the front-end's own signature is as it was


def test_device_functions_refuse_without_a_gpu_tensor():
    x = torch.zeros(2, 3, 4, 5, 2)
    with pytest.raises(CineHipError, match="aug"):
        A.warp(x, IDENT)
    with pytest.raises(CineHipError, match="GPU tensor"):
        A.warp(x, A.identity())
    with pytest.raises(CineHipError, match="expected"):
        A.warp(torch.zeros(3, 4, 5), A.identity())
    with pytest.raises(CineHipError, match="aug"):
        A.augment_example(x, None)
    with pytest.raises(CineHipError, match="sens"):
        A.warp_maps(torch.zeros(4, 5, 2), A.identity())
