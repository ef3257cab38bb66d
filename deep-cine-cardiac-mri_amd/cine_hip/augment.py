"""Physics-aware training augmentation on the device (MRAugment: Fabian et al., ICML 2021).  No reference counterpart: the reference
trains without augmentation.

The fully sampled complex coil images are transformed, taken back to k-space and undersampled, and the target is formed from the
transformed images, so the measurement model still holds for the augmented example:

``Augmentation``     one transform of a cine slice: a 2 x 3 inverse affine map in pixels about the image centre, a cyclic shift /
                     reversal of the cardiac cycle, the interpolation mode and the border rule.  Immutable; ``from_params`` builds it
                     from rotation, scale, shear, translation, flips and quarter turns, ``identity`` and ``compose`` do what they say.
``sample``           draws one from ranges (a seed per example makes a run repeatable), ``schedule`` is MRAugment's probability ramp.
``warp``             cine_affine_warp (csrc/augment_kernels.hip) on (t, c, h, w, 2) or (c, h, w, 2): ONE launch for all frames and
                     coils, in the layout every other kernel reads -- no permute, no materialised grid.
``warp_maps``        sensitivity maps under the spatial part of the transform, renormalised to unit root-sum-of-squares.
``augment_example``  the chain: warp -> k-space of the warped images -> mask -> maps -> target, nothing on the host.
``prepare_example``  ``frontend.prepare_example`` with one more keyword, ``augment=``: the reference's sample tuple of the augmented
                     example; ``augment=None`` IS ``frontend.prepare_example``.  (It lives here, not in ``frontend``: that function's
                     signature is pinned by the suite with ``whitener`` last.)

The convention of the map is ``torch.nn.functional.grid_sample(align_corners=False)`` behind ``affine_grid`` (include/cine_hip.h has the
formulae).  Resampling interpolates: it lowers and correlates the noise of the images, bicubic less than bilinear.  Not built:
per-frame transforms, a gradient of the warp, anti-aliasing for strong down-scaling.
"""
import math
import numbers
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import CineHipError, check, lib

MODES = ("bilinear", "bicubic")
BORDERS = ("zeros", "reflect")
MAX_A = 1024.0                                   # the limits of cine_affine_warp
MAX_B = 2.0 ** 20
MAX_SIDE = 4096


def _is_int(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


@dataclass(frozen=True)
class Augmentation:
    """``matrix``: ((a_yy, a_yx, b_y), (a_xy, a_xx, b_x)) float64, the INVERSE map in pixels about the image centre: the output pixel
    at offset (dy, dx) from the centre reads the source at offset (a_yy dy + a_yx dx + b_y, a_xy dy + a_xx dx + b_x).  ``t_shift``,
    ``t_reverse``: output frame f reads source frame (f + t_shift) mod t, or (t_shift - f) mod t when reversed (any integer shift: it is
    reduced by the frame count where the transform is applied).  ``mode``: "bilinear" | "bicubic"; ``border``: "zeros" | "reflect".
    Validated with the limits of cine_affine_warp (finite, |a| <= 1024, |b| <= 2^20); a CineHipError names the field."""
    matrix: Tuple[Tuple[float, float, float], Tuple[float, float, float]] = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    t_shift: int = 0
    t_reverse: bool = False
    mode: str = "bicubic"
    border: str = "reflect"

    def __post_init__(self):
        try:
            m = np.array(self.matrix, dtype=np.float64)
        except (TypeError, ValueError):
            m = None
        if m is None or m.shape != (2, 3):
            raise CineHipError("Augmentation: matrix: expected 2 x 3 numbers ((a_yy, a_yx, b_y), (a_xy, a_xx, b_x))")
        if not np.isfinite(m).all():
            raise CineHipError("Augmentation: matrix: an entry is not finite")
        if (np.abs(m[:, :2]) > MAX_A).any():
            raise CineHipError(f"Augmentation: matrix: a linear entry exceeds {MAX_A:g} in size")
        if (np.abs(m[:, 2]) > MAX_B).any():
            raise CineHipError(f"Augmentation: matrix: an offset exceeds 2^20 = {MAX_B:g} pixels in size")
        object.__setattr__(self, "matrix", tuple(tuple(float(v) for v in row) for row in m))
        if not _is_int(self.t_shift):
            raise CineHipError(f"Augmentation: t_shift: expected an integer, got {self.t_shift!r}")
        object.__setattr__(self, "t_shift", int(self.t_shift))
        if not isinstance(self.t_reverse, (bool, np.bool_)):
            raise CineHipError(f"Augmentation: t_reverse: expected a bool, got {self.t_reverse!r}")
        object.__setattr__(self, "t_reverse", bool(self.t_reverse))
        if self.mode not in MODES:
            raise CineHipError(f"Augmentation: mode: {self.mode!r} is not one of {MODES}")
        if self.border not in BORDERS:
            raise CineHipError(f"Augmentation: border: {self.border!r} is not one of {BORDERS}")

    # ------------------------------------------------------------------ views
    def array(self) -> np.ndarray:
        """The inverse map as a fresh (2, 3) float64 array."""
        return np.array(self.matrix, dtype=np.float64)

    def homogeneous(self) -> np.ndarray:
        """The inverse map as a (3, 3) float64 matrix on (dy, dx, 1)."""
        return np.vstack([self.array(), [0.0, 0.0, 1.0]])

    def frame_map(self, frames: int) -> np.ndarray:
        """The source frame of every output frame: an int64 permutation of range(frames)."""
        if not _is_int(frames) or frames < 1:
            raise CineHipError(f"Augmentation.frame_map: frames = {frames!r} must be a positive integer")
        f = np.arange(frames, dtype=np.int64)
        return np.mod(self.t_shift - f if self.t_reverse else f + self.t_shift, frames)

    def spatial(self, mode: Optional[str] = None, border: Optional[str] = None) -> "Augmentation":
        """The same map without the temporal part (and, if given, another mode / border)."""
        return Augmentation(self.matrix, 0, False, mode or self.mode, border or self.border)

    def moves_pixels_only(self, h: int, w: int) -> bool:
        """Whether every source coordinate on an h x w plane is integral: the linear part a signed permutation, the offsets integers
        (and, where the axes swap, h - w even).  Resampling is then a copy of pixels, whatever the mode."""
        (ayy, ayx, by), (axy, axx, bx) = self.matrix
        straight = abs(ayy) == 1.0 and abs(axx) == 1.0 and ayx == 0.0 and axy == 0.0
        swapped = abs(ayx) == 1.0 and abs(axy) == 1.0 and ayy == 0.0 and axx == 0.0 and (h - w) % 2 == 0
        return (straight or swapped) and by == math.floor(by) and bx == math.floor(bx)

    def is_identity(self) -> bool:
        return self.matrix == ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)) and self.t_shift == 0 and not self.t_reverse

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_params(h: int, w: int, rotation_deg: float = 0.0, scale=(1.0, 1.0), shear_deg=(0.0, 0.0), translate=(0.0, 0.0),
                    flip_h: bool = False, flip_v: bool = False, rot90: int = 0, t_shift: int = 0, t_reverse: bool = False,
                    mode: str = "bicubic", border: str = "reflect") -> "Augmentation":
        """The transform with the FORWARD map, on offsets (dy, dx) from the image centre ((h - 1) / 2, (w - 1) / 2),

            F = T(translate) R(rotation_deg) Sh(shear_deg) S(scale) Q^rot90 Flip

        applied right to left: flips first (``flip_h`` mirrors along w like ``torch.flip`` of the w axis, ``flip_v`` along h), then
        ``rot90`` quarter turns Q = [[0, -1], [1, 0]] (``torch.rot90(x, rot90, (h axis, w axis))``; needs h == w), the scaling
        diag(scale_y, scale_x) (> 1 magnifies), the shear [[1, tan s_y], [tan s_x, 1]], the rotation [[cos, -sin], [sin, cos]] (in the
        sense of ``rot90``: 90 degrees is one quarter turn), and the translation by (t_y, t_x) pixels.  Stored is F^-1, the product of
        the factors' own inverses in the opposite order: flips, quarter turns and integer translations are built from integers, never
        from cos(pi / 2), and a parameter left at its default contributes an exact identity."""
        return Augmentation(tuple(map(tuple, affine_matrices(h, w, rotation_deg, scale, shear_deg, translate, flip_h, flip_v, rot90)[1][:2])),
                            t_shift, t_reverse, mode, border)


def _pair_of(v, name: str) -> Tuple[float, float]:
    if isinstance(v, numbers.Real):
        v = (v, v)
    try:
        a, b = (float(x) for x in v)
    except (TypeError, ValueError):
        raise CineHipError(f"Augmentation.from_params: {name}: expected a number or a pair (y, x), got {v!r}") from None
    if not (math.isfinite(a) and math.isfinite(b)):
        raise CineHipError(f"Augmentation.from_params: {name}: {v!r} is not finite")
    return a, b


def _lin(m) -> np.ndarray:
    out = np.eye(3)
    out[:2, :2] = m
    return out


def _shift(ty: float, tx: float) -> np.ndarray:
    out = np.eye(3)
    out[0, 2], out[1, 2] = ty, tx
    return out


def affine_matrices(h: int, w: int, rotation_deg: float = 0.0, scale=(1.0, 1.0), shear_deg=(0.0, 0.0), translate=(0.0, 0.0),
                    flip_h: bool = False, flip_v: bool = False, rot90: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(F, F^-1) of ``Augmentation.from_params``: (3, 3) float64 matrices on (dy, dx, 1), each the product of its own factors."""
    what = "Augmentation.from_params"
    if not (_is_int(h) and _is_int(w) and 1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise CineHipError(f"{what}: h, w: ({h!r}, {w!r}) must be integers in 1..{MAX_SIDE}")
    if not _is_int(rot90):
        raise CineHipError(f"{what}: rot90: expected an integer number of quarter turns, got {rot90!r}")
    k = int(rot90) % 4
    if k and h != w:
        raise CineHipError(f"{what}: rot90: quarter turns need a square image, got {h} x {w}")
    if not (isinstance(rotation_deg, numbers.Real) and math.isfinite(rotation_deg)):
        raise CineHipError(f"{what}: rotation_deg: {rotation_deg!r} is not a finite number")
    sy, sx = _pair_of(scale, "scale")
    if sy == 0.0 or sx == 0.0:
        raise CineHipError(f"{what}: scale: {scale!r} has a zero factor")
    shy, shx = (math.tan(math.radians(v)) for v in _pair_of(shear_deg, "shear_deg"))
    det = 1.0 - shy * shx
    if not (abs(shy) <= MAX_A and abs(shx) <= MAX_A) or abs(det) < 1e-6:
        raise CineHipError(f"{what}: shear_deg: {shear_deg!r} is a singular or unbounded shear")
    ty, tx = _pair_of(translate, "translate")
    fy, fx = (-1.0 if flip_v else 1.0), (-1.0 if flip_h else 1.0)
    flip = _lin([[fy, 0.0], [0.0, fx]])
    quarter = (np.eye(2), np.array([[0.0, -1.0], [1.0, 0.0]]), np.array([[-1.0, 0.0], [0.0, -1.0]]), np.array([[0.0, 1.0], [-1.0, 0.0]]))
    th = math.radians(float(rotation_deg))
    cs, sn = (1.0, 0.0) if rotation_deg == 0 else (math.cos(th), math.sin(th))
    fwd = _shift(ty, tx) @ _lin([[cs, -sn], [sn, cs]]) @ _lin([[1.0, shy], [shx, 1.0]]) @ _lin([[sy, 0.0], [0.0, sx]]) @ _lin(quarter[k]) @ flip
    inv = (flip @ _lin(quarter[(4 - k) % 4]) @ _lin([[1.0 / sy, 0.0], [0.0, 1.0 / sx]]) @ _lin(np.array([[1.0, -shy], [-shx, 1.0]]) / det)
           @ _lin([[cs, sn], [-sn, cs]]) @ _shift(-ty, -tx))
    return fwd + 0.0, inv + 0.0                  # + 0.0: no negative zeros from the products


def identity(mode: str = "bicubic", border: str = "reflect") -> Augmentation:
    """The transform that changes nothing: ``warp`` of it is a copy, bit for bit."""
    return Augmentation(mode=mode, border=border)


def compose(a: Augmentation, b: Augmentation, mode: Optional[str] = None, border: Optional[str] = None) -> Augmentation:
    """``a`` then ``b`` as ONE transform: forward map F_b F_a, so the stored inverse is M_a M_b, and the frame maps composed likewise.
    Mode and border are ``a``'s unless given.  One resampling under the composed map is not bit-equal to two in a row (each interpolates);
    for flips, quarter turns and integer shifts it is."""
    if not (isinstance(a, Augmentation) and isinstance(b, Augmentation)):
        raise CineHipError("compose: expected two Augmentation objects")
    m = a.homogeneous() @ b.homogeneous() + 0.0
    sa = -1 if a.t_reverse else 1
    return Augmentation(tuple(map(tuple, m[:2])), a.t_shift + sa * b.t_shift, a.t_reverse != b.t_reverse, mode or a.mode, border or a.border)


def _rng_of(rng_or_seed) -> np.random.Generator:
    if isinstance(rng_or_seed, np.random.Generator):
        return rng_or_seed
    if _is_int(rng_or_seed):
        return np.random.default_rng([int(rng_or_seed)])
    try:
        seq = [int(v) for v in rng_or_seed]
    except (TypeError, ValueError):
        seq = None
    if not seq or any(v < 0 for v in seq):
        raise CineHipError(f"sample: rng_or_seed: expected a numpy Generator, a non-negative int or a sequence like (seed, epoch, index), "
                           f"got {rng_or_seed!r}")
    return np.random.default_rng(seq)


def sample(rng_or_seed, h: int, w: int, p: float = 0.55, frames: Optional[int] = None, *, rotation: float = 180.0, shear: float = 15.0,
           scale: float = 0.25, translate: Sequence[float] = (0.08, 0.125), weight_rotation: float = 1.0, weight_shear: float = 1.0,
           weight_scale: float = 1.0, weight_translate: float = 1.0, weight_flip_h: float = 0.5, weight_flip_v: float = 0.5,
           weight_rot90: float = 0.5, weight_t_shift: float = 0.5, weight_t_reverse: float = 0.5, mode: str = "bicubic",
           border: str = "reflect") -> Augmentation:
    """One random transform of an h x w slice.  Each elementary transform is drawn independently with probability ``p`` times its
    weight (clipped to 1): a rotation uniform in +-``rotation`` degrees, shears uniform in +-``shear`` degrees per axis, an isotropic
    scaling uniform in 1 +- ``scale``, a translation uniform in +-``translate`` = (fraction of h, fraction of w), the two flips, one to
    three quarter turns (square slices only), and -- with ``frames`` -- a cyclic shift of the cardiac cycle uniform over the frames and
    its reversal.  They combine as in ``Augmentation.from_params``.

    The default ranges and weights are MRAugment's settings for fastMRI knee data as remembered -- rotation +-180 degrees, shearing
    +-15 degrees, scaling +-0.25, translation 12.5 % of the width and 8 % of the height, flips and quarter turns at weight 0.5 -- not
    checked against its published configuration and NOT tuned on cine data; the temporal weights (0.5) are this package's guess.
    Tune them per data set, with ``schedule`` for ``p``.

    ``rng_or_seed``: a ``numpy.random.Generator``, or an int / a sequence of ints for ``numpy.random.default_rng``: pass
    ``(seed, epoch, index)`` and the transform of every example of every epoch is repeatable.  Every random number is drawn whether its
    transform is used or not, so one transform's probability does not move the others' values."""
    rng = _rng_of(rng_or_seed)
    if not (isinstance(p, numbers.Real) and 0.0 <= p <= 1.0):
        raise CineHipError(f"sample: p: {p!r} is not a probability")
    if frames is not None and (not _is_int(frames) or frames < 1):
        raise CineHipError(f"sample: frames: {frames!r} must be a positive integer or None")
    fy, fx = _pair_of(translate, "translate")
    u = rng.random(9)                                                        # the decisions, in the order below
    v = rng.uniform(-1.0, 1.0, 6)                                            # rotation, shear y, shear x, scale, translate y, translate x
    quarter = int(rng.integers(1, 4))
    shift = int(rng.integers(0, frames)) if frames else 0
    on = lambda i, wgt: bool(u[i] < min(1.0, p * float(wgt)))
    kw = {}
    if on(0, weight_rotation):
        kw["rotation_deg"] = float(v[0] * rotation)
    if on(1, weight_shear):
        kw["shear_deg"] = (float(v[1] * shear), float(v[2] * shear))
    if on(2, weight_scale):
        s = 1.0 + float(v[3] * scale)
        kw["scale"] = (s, s)
    if on(3, weight_translate):
        kw["translate"] = (float(v[4] * fy * h), float(v[5] * fx * w))
    kw["flip_h"], kw["flip_v"] = on(4, weight_flip_h), on(5, weight_flip_v)
    if on(6, weight_rot90) and h == w:
        kw["rot90"] = quarter
    if frames and on(7, weight_t_shift):
        kw["t_shift"] = shift
    if frames and on(8, weight_t_reverse):
        kw["t_reverse"] = True
    return Augmentation.from_params(h, w, mode=mode, border=border, **kw)


def schedule(epoch: float, epochs: float, p_max: float = 0.55, decay: float = 5.0) -> float:
    """MRAugment's exponential ramp of the augmentation probability: ``p_max (1 - exp(-decay e / E)) / (1 - exp(-decay))``: 0 at epoch
    0, ``p_max`` at epoch ``epochs``, monotone (early epochs see the real data, late ones fight overfitting)."""
    if not (epochs > 0 and 0 <= epoch <= epochs):
        raise CineHipError(f"schedule: epoch {epoch!r} must lie in [0, epochs = {epochs!r}], epochs > 0")
    if not (0.0 <= p_max <= 1.0 and decay > 0):
        raise CineHipError(f"schedule: p_max {p_max!r} must be a probability and decay {decay!r} positive")
    return float(p_max * (1.0 - math.exp(-decay * epoch / epochs)) / (1.0 - math.exp(-decay)))


# ====================================================================== the device side
def _need(aug, what: str) -> Augmentation:
    if not isinstance(aug, Augmentation):
        raise CineHipError(f"{what}: aug: expected an Augmentation, got {type(aug).__name__}")
    return aug


def warp(images, aug: Augmentation, out=None):
    """``images`` under ``aug``: (t, c, h, w, 2) or (c, h, w, 2) float32 pairs, or (t, c, h, w) / (c, h, w) complex64, contiguous, on the
    GPU; the result has the input's form.  One launch of cine_affine_warp; every element of the result is written.  ``out``: the
    result's place (same form, contiguous, not overlapping the input).  Without a frame axis the transform's temporal part must be
    trivial.  Not differentiable."""
    _need(aug, "warp")
    if not isinstance(images, torch.Tensor):
        raise TypeError("warp: images: expected a tensor")
    if images.requires_grad:
        raise CineHipError("warp: not differentiable; detach the images")
    cplx = images.is_complex()
    if cplx:
        if images.dtype != torch.complex64:
            raise CineHipError(f"warp: images are {images.dtype}; expected complex64 or float32 pairs")
        x = torch.view_as_real(images if images.is_contiguous() else images.contiguous())
    else:
        x = images
    if x.dim() not in (4, 5) or x.shape[-1] != 2:
        raise CineHipError(f"warp: images {tuple(images.shape)} {images.dtype}; expected (t, c, h, w, 2) / (c, h, w, 2) float32 or "
                           "(t, c, h, w) / (c, h, w) complex64")
    x = ops._dev(x, "warp images")
    frames = x.shape[0] if x.dim() == 5 else 1
    c, h, w = x.shape[-4], x.shape[-3], x.shape[-2]
    if min(frames, c, h, w) < 1:
        raise CineHipError(f"warp: images {tuple(images.shape)}: an empty axis")
    if x.dim() == 4 and (aug.t_reverse or aug.t_shift):
        raise CineHipError("warp: t_shift / t_reverse: the images have no frame axis")
    if out is None:
        res = torch.empty_like(x)
    else:
        if not (isinstance(out, torch.Tensor) and out.device == images.device and out.dtype == images.dtype and out.is_contiguous()
                and out.shape == images.shape):
            raise CineHipError(f"warp: out must be a contiguous {images.dtype} tensor {tuple(images.shape)} on the images' device")
        res = torch.view_as_real(out) if cplx else out
    (ayy, ayx, by), (axy, axx, bx) = aug.matrix
    check(lib().cine_affine_warp(x.data_ptr(), res.data_ptr(), frames, c, h, w, ayy, ayx, by, axy, axx, bx, MODES.index(aug.mode),
                                 BORDERS.index(aug.border), aug.t_shift % frames, int(aug.t_reverse), ops._stream()), "cine_affine_warp")
    if out is not None:
        return out
    return torch.view_as_complex(res) if cplx else res


def warp_maps(sens, aug: Augmentation):
    """Sensitivity maps (c, h, w, 2) float32 (or (c, h, w) complex64) under the spatial part of ``aug``, bilinear with ``aug``'s border,
    renormalised: where the root-sum-of-squares of the warped maps is >= 0.5 they are divided by it, elsewhere they are zero.  ESPIRiT
    maps have RSS 1 inside the object and 0 outside, and interpolation across that edge gives values in between: 0.5 is the edge.
    A map that only moves pixels -- flips, quarter turns, integer shifts, the identity -- mixes nothing: the warped maps are returned as
    they are, every pixel the bits of its source (or zero outside under border "zeros")."""
    _need(aug, "warp_maps")
    cplx = isinstance(sens, torch.Tensor) and sens.is_complex()
    if not isinstance(sens, torch.Tensor) or sens.dim() != (3 if cplx else 4):
        raise CineHipError("warp_maps: sens: expected (c, h, w, 2) float32 or (c, h, w) complex64")
    m = warp(sens, aug.spatial(mode="bilinear"))
    if aug.moves_pixels_only(*(sens.shape[-2:] if cplx else sens.shape[-3:-1])):
        return m
    r = torch.view_as_real(m) if cplx else m
    rss = r.square().sum(dim=(0, 3), keepdim=True).sqrt()
    keep = rss >= 0.5
    r = torch.where(keep, r / torch.where(keep, rss, torch.ones_like(rss)), torch.zeros_like(r)).contiguous()
    return torch.view_as_complex(r) if cplx else r


def augment_example(filt, aug: Augmentation, mask=None, sens=None, crop_target=(180, 180), *, ecalib_r: int = 200,
                    espirit_method: str = "eigh"):
    """One augmented training example from the filtered crop images ``filt`` (t, c, X, Y, 2) that ``frontend.prepare_slice`` returns:
    ``(kspace, sens, target)`` on the device.  ``kspace`` (t, c, X, Y, 2) is the k-space of the warped images
    (``frontend._to_kspace_hip``), masked with ``ops.apply_mask`` when ``mask`` (uint8, its forms) is given; ``sens`` (c, X, Y, 2) is
    ``warp_maps`` of the given maps, or with ``sens=None`` a fresh calibration of the time average of that k-space
    (``frontend.ecalib(r=ecalib_r, method=espirit_method)``); ``target`` (t, cx, cy) is ``frontend.combine_target`` of the warped images
    with those maps.  Nothing goes to the host (``espirit_method="eigh"`` lets torch.linalg.eigh check its result there)."""
    from . import frontend
    _need(aug, "augment_example")
    if not (isinstance(filt, torch.Tensor) and filt.dim() == 5 and filt.shape[-1] == 2):
        raise CineHipError("augment_example: filt: expected (t, c, X, Y, 2) float32 pairs (frontend.prepare_slice's second result)")
    images = warp(filt, aug)
    kspace = frontend._to_kspace_hip(images)
    if mask is not None:
        kspace = ops.apply_mask(kspace, mask)
    if sens is None:
        time_avg = torch.view_as_complex(kspace.mean(dim=0, keepdim=True).contiguous()).permute(0, 2, 3, 1)     # (1, X, Y, coil)
        maps = torch.view_as_real(frontend.ecalib(time_avg, r=ecalib_r, method=espirit_method).permute(2, 0, 1).contiguous()).contiguous()
    else:
        maps = warp_maps(torch.view_as_real(sens).contiguous() if sens.is_complex() else sens, aug)
    target = frontend.combine_target(images, maps, crop_target)
    return kspace, maps, target


def prepare_example(source, mask=None, sens=None, fname: str = "", crop_shape=(200, 200), crop_target=(180, 180), n_slices: int = 15,
                    filter_size=(0.7, 0.0, 0.3, 0.3), scaling: float = 1e6, ecalib_r: int = 200, virtual_coils: Optional[int] = None,
                    coil_matrix=None, cc_region: int = 24, espirit_method: str = "eigh", cc_method: str = "eigh", whitener=None,
                    augment: Optional[Augmentation] = None):
    """``frontend.prepare_example`` -- ``SliceDataset.__getitem__`` of the reference on the device, its arguments and its tuple (kspace
    (t, coil, X, Y) complex64, mask, target (t, cx, cy) float32, attrs, fname, dataslice) as numpy arrays -- with ``augment=`` behind
    them.  ``None``: the call is handed to ``frontend.prepare_example`` as it is, its path and its bits.  An ``Augmentation``: the same
    front part (``frontend.prepare_slice``), then ``augment_example``: the filtered crop images are warped, k-space is the transform of
    the warped images, given maps are warped with them (``warp_maps``; with ``sens=None`` the calibration runs on the augmented
    k-space), and the target is formed from the warped images.  ``mask`` is passed through, as there."""
    from . import frontend
    if augment is None:
        return frontend.prepare_example(source, mask, sens, fname, crop_shape, crop_target, n_slices, filter_size, scaling, ecalib_r,
                                        virtual_coils, coil_matrix, cc_region, espirit_method, cc_method, whitener)
    _need(augment, "prepare_example")
    if hasattr(source, "keys") and "y" in source:
        raw = np.asarray(source["y"])
        if mask is None and "mask" in source:
            mask = np.asarray(source["mask"])
    else:
        raw = source
    if not torch.cuda.is_available():
        raise CineHipError("prepare_example: the front-end kernels need a GPU (no CPU fallback)")
    y = torch.as_tensor(raw).to(torch.complex64).cuda()
    _, filt = frontend.prepare_slice(y, crop_shape, n_slices, filter_size, scaling, virtual_coils, coil_matrix, cc_region, cc_method, whitener)
    if sens is not None and (virtual_coils is not None or coil_matrix is not None) and tuple(sens.shape)[0] != filt.shape[1]:
        raise ValueError(f"sens has {tuple(sens.shape)[0]} coils, the compressed data {filt.shape[1]}")
    given = None if sens is None else torch.as_tensor(sens).to(torch.complex64).cuda()
    kspace, _, target = augment_example(filt, augment, None, given, crop_target, ecalib_r=ecalib_r, espirit_method=espirit_method)
    return torch.view_as_complex(kspace.contiguous()).cpu().numpy(), mask, target.cpu().numpy(), {}, fname, 0
