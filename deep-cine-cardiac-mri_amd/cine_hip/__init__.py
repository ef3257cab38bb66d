"""cine_hip: host-side bindings of the MI355X cine-reconstruction kernels.

The numerics live in ``csrc/*.hip`` (hand-written gfx950 kernels) behind the
C ABI declared in ``include/cine_hip.h``; this package loads
``libcine_hip.so`` with ctypes and passes raw device pointers and the caller's
HIP stream.  There is no CPU fallback: any compute entry point raises
``CineHipError`` when the library or a GPU is missing.
"""
import os as _os

# The HIP runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4).  The training path runs its weight gradients on a side
# stream (csrc/grad.h: SideLane) and RCCL brings streams of its own: with four queues the side stream ends up sharing a queue with the
# main one and the overlap is gone (cfg-2 training step 40.4 -> 45.7 ms once a process group exists).  Takes effect only if the runtime
# has not been initialised yet; an explicit setting of the user wins.
def _hw_queue_default() -> None:
    import sys
    import warnings
    if "GPU_MAX_HW_QUEUES" in _os.environ:
        return
    _os.environ["GPU_MAX_HW_QUEUES"] = "16"
    torch = sys.modules.get("torch")          # never imports torch itself: the question is whether the runtime is ALREADY up
    try:
        started = bool(torch is not None and torch.cuda.is_initialized())
    except Exception:                          # pragma: no cover
        started = False
    if started:
        warnings.warn("cine_hip was imported after the HIP runtime had been initialised and GPU_MAX_HW_QUEUES is not set: the runtime keeps its "
                      "default of 4 hardware queues, on which the weight-gradient side stream, the U-Net branches and RCCL's streams share queues "
                      "(measured: cfg-2 training step 40.4 -> 45.7 ms).  Export GPU_MAX_HW_QUEUES=16 before the first GPU call, or import "
                      "reconstruction.models / cine_hip first.", RuntimeWarning, stacklevel=3)


_hw_queue_default()

from . import synth  # noqa: F401,E402  (host-only, numpy)

__all__ = ["synth", "fista_momentum", "kt_sparse_sense", "KtSparseSense", "low_rank_plus_sparse", "LowRankPlusSparse", "total_variation",
           "TotalVariation", "locally_low_rank", "LocallyLowRank", "lattice_mask", "plan_lattice", "calibration_data", "grappa_weights", "grappa",
           "Grappa", "plan_gaps", "gap_table", "grappa_weights_gaps", "grappa_apply_gaps", "grappa_image_weights",
           "grappa_gfactor_from_weights", "grappa_noise_maps"]

_CLASSICAL = ("fista_momentum", "kt_sparse_sense", "KtSparseSense", "low_rank_plus_sparse", "LowRankPlusSparse", "total_variation",
              "TotalVariation", "locally_low_rank", "LocallyLowRank")
_GRAPPA = ("lattice_mask", "plan_lattice", "calibration_data", "grappa_weights", "Grappa", "plan_gaps", "gap_table", "grappa_weights_gaps",
           "grappa_apply_gaps", "grappa_image_weights", "grappa_gfactor_from_weights", "grappa_noise_maps")


def __getattr__(name):
    # the weight-free baselines (cine_hip.classical), imported on first use: the package import itself stays host-only
    if name in _CLASSICAL:
        from . import classical
        return getattr(classical, name)
    if name in ("noise", "gating", "augment", "grappa"):    # cine_hip.noise: pseudo-replica noise maps; cine_hip.gating: retrospective
        import importlib                          # gating; cine_hip.augment: training augmentation; cine_hip.grappa: the GRAPPA / TGRAPPA
        return importlib.import_module("." + name, __name__)    # baseline (the module; its function is cine_hip.grappa.grappa) -- on first use
    if name in _GRAPPA:
        import importlib
        return getattr(importlib.import_module(".grappa", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
