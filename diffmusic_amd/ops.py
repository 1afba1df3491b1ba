"""PyTorch-ROCm custom ops `torch.ops.diffmusic_hip.*`: TORCH_LIBRARY wrappers over the C ABI,
compiled from csrc_torch/torch_ops.cpp into lib/libdiffmusic_torch_ops.so and loaded with `torch.ops.load_library`.

    from diffmusic_amd import ops
    prev, x0 = ops.hip.sched_update(1, x, eps, x0, g0, inv_scale, None, a_t, a_p, sigma, rate, 1e-8, False)

The facades (`Scheduler.step`, `Pipeline.__call__`, the operators, the engines) call `ops.hip.<name>` and nothing else: it resolves,
per call, to `torch.ops.diffmusic_hip.<name>` (default) or to the ctypes function of the same name and signature
(`_ctypes_ops.py`, also exposed as `ops.ctypes_hip` for tests); both end in the same `extern "C"` launchers on torch's current HIP
stream.  DMX_TORCH_OPS=0 selects the ctypes binding; so does DMX_LIB_PATH (a dev build of libdiffmusic_hip.so: the op library links
the in-tree one) and an op library that cannot be loaded (missing, or built against another torch): one warning, then ctypes -- the
same HIP kernels either way.  This module is the only place that knows which binding carries a launch: no facade names a binding.

There is one op per operation.  What an operation can do beyond its plain form -- a caller-owned or strided output (`out`, `dwav`,
`grad_out`), prediction type / clip range, the guidance pair's noise and clip thresholds, a vocoder dead span, the U-Net's context
tensors and output channels -- is a defaulted argument of that op, identical in both bindings (tests/test_abi.py compares names,
order, keyword-only split and defaults).  The C ABI keeps its additive ladder (_ex / _shaped / _ctx / _dead) for C callers; the op
layer calls the longest rung.  Neither binding has a CPU fallback: without libdiffmusic_hip.so everything raises."""
import inspect
import os
import warnings

import torch

from . import _ctypes_ops as ctypes_hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdiffmusic_torch_ops.so")
USE_TORCH_OPS = os.environ.get("DMX_TORCH_OPS", "1") not in ("", "0")
_loaded = False

# every registered op has a ctypes function of its name (tests/test_abi.py compares the two signatures)
OP_NAMES = tuple(n for n, f in vars(ctypes_hip).items() if inspect.isfunction(f) and not n.startswith("_"))
_usable = None


def load():
    """Loads the op library once (raises if it is missing: build it with `python -m diffmusic_amd.build`)."""
    global _loaded
    if not _loaded:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -m diffmusic_amd.build` (no CPU fallback)")
        from . import _lib
        _lib.lib()                                   # libdiffmusic_hip.so first (the op library links it by rpath $ORIGIN)
        torch.ops.load_library(LIB_PATH)             # (its TORCH_LIBRARY init refuses a libdiffmusic_hip.so of another C-ABI version)
        if int(torch.ops.diffmusic_hip.abi_version()) != _lib.ABI_VERSION:
            raise RuntimeError(f"libdiffmusic_torch_ops.so was compiled against C-ABI version {int(torch.ops.diffmusic_hip.abi_version())}, "
                               f"this package expects {_lib.ABI_VERSION}: rebuild it with `python -m diffmusic_amd.build`")
        _loaded = True
    return torch.ops.diffmusic_hip


def enabled():
    """True when the facade should call torch.ops.diffmusic_hip.* (default), False for the ctypes binding: DMX_TORCH_OPS=0, or the
    op library failed to load (warned about once; the HIP library itself is still required)."""
    global _usable
    if not USE_TORCH_OPS:
        return False
    if os.environ.get("DMX_LIB_PATH"):
        # a dev A/B build of libdiffmusic_hip.so is selected for the ctypes binding; the op library is linked (rpath) against the
        # in-tree one, so going through it would silently measure the other library's kernels
        return False
    if _usable is None:
        try:
            load()
            _usable = True
        except (RuntimeError, OSError) as e:
            warnings.warn(f"torch.ops.diffmusic_hip is unavailable ({e}); using the ctypes binding of the same HIP entry points. "
                          "Rebuild with `python -m diffmusic_amd.build`.", RuntimeWarning, stacklevel=2)
            _usable = False
    return _usable


class _Hip:
    """`ops.hip.<name>`: the op of that name in the binding that is in force for this call."""

    def __getattr__(self, name):
        return getattr(load() if enabled() else ctypes_hip, name)


hip = _Hip()
