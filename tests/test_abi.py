"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/diffmusic_hip.h declares
(no compute calls without a GPU)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "diffmusic_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dmx_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_loads_and_exports_all_declared_symbols():
    from diffmusic_amd.build import build_library
    lib = build_library()
    assert os.path.exists(lib)
    h = ctypes.CDLL(lib)
    names = _declared_symbols()
    assert len(names) >= 35
    missing = [n for n in names if not hasattr(h, n)]
    assert not missing, missing
    h.dmx_abi_version.restype = ctypes.c_int
    assert h.dmx_abi_version() == 4
    assert h.dmx_act_dtype() in (0, 1)


def test_binding_signatures_cover_the_header():
    from diffmusic_amd import _lib
    bound = set(_lib._SIGS)
    declared = set(_declared_symbols())
    assert declared <= bound, sorted(declared - bound)


def test_product_fails_loudly_without_library(monkeypatch, tmp_path):
    from diffmusic_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    try:
        _lib.lib()
        raise AssertionError("expected a RuntimeError")
    except RuntimeError as e:
        assert "no CPU fallback" in str(e)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "diffmusic_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), os.path.join(dp, f)


def test_torch_op_library_loads_and_registers_every_stage_op(monkeypatch, tmp_path):
    """TORCH_LIBRARY(diffmusic_hip) layer: builds, loads without a GPU, registers all stage ops, fails
    loudly when the library is missing, and refuses CPU tensors (no CPU fallback)."""
    import pytest
    import torch
    from diffmusic_amd.build import build_torch_ops
    from diffmusic_amd import ops
    assert os.path.exists(build_torch_ops())
    h = ops.load()
    for name in ops.OP_NAMES:
        assert hasattr(h, name), name
        assert str(getattr(h, name).default._schema).startswith(f"diffmusic_hip::{name}(")
    for want in ("unet_fwd", "vae_dec_fwd", "vae_dec_bwd", "hifigan_fwd", "hifigan_bwd", "logmel_fwd", "logmel_bwd", "stft_mag_fwd",
                 "stft_mag_bwd", "melscale_fwd", "resample_fwd", "resample_bwd", "mask_mul", "l2norm", "sched_update", "randn_philox"):
        assert want in ops.OP_NAMES                                   # the op list of SURVEY.md section 8b.4
    with pytest.raises(RuntimeError, match="GPU tensor"):
        h.sched_pred_x0(torch.zeros(2, 4), torch.zeros(2, 4), 0.5)
    monkeypatch.setattr(ops, "_loaded", False)
    monkeypatch.setattr(ops, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.load()


def test_ctypes_ops_have_the_positional_signatures_of_the_registered_ops():
    """The two bindings are one surface: every op registered in csrc_torch/torch_ops.cpp has a function of its name in
    diffmusic_amd/_ctypes_ops.py with the schema's arguments: the same names in the same order, the same positional / keyword-only
    split and the same default values, so a call written for one is a call of the other."""
    import inspect
    from diffmusic_amd.build import build_torch_ops
    from diffmusic_amd import ops
    assert os.path.exists(build_torch_ops())
    h = ops.load()
    src = open(os.path.join(ROOT, "diffmusic_amd", "csrc_torch", "torch_ops.cpp")).read()
    registered = re.findall(r'm\.def\("([A-Za-z0-9_]+)\(', src)
    assert len(registered) >= 26 and len(set(registered)) == len(registered)
    assert sorted(registered) == sorted(ops.OP_NAMES)
    P = inspect.Parameter
    defaulted = 0
    for name in ops.OP_NAMES:
        want = [(a.name, a.kwarg_only, a.has_default_value(), a.default_value if a.has_default_value() else None)
                for a in getattr(h, name).default._schema.arguments]
        params = list(inspect.signature(getattr(ops.ctypes_hip, name)).parameters.values())
        assert all(p.kind in (P.POSITIONAL_OR_KEYWORD, P.KEYWORD_ONLY) for p in params), name
        got = [(p.name, p.kind == P.KEYWORD_ONLY, p.default is not P.empty, None if p.default is P.empty else p.default) for p in params]
        assert got == want, (name, got, want)
        assert all(type(g[3]) is type(w[3]) for g, w in zip(got, want)), (name, got, want)      # 0 is not 0.0 is not False
        defaulted += sum(w[2] for w in want)
    assert defaulted >= 20                                              # the schemas do carry defaults for this to compare


def test_only_ops_py_names_a_binding():
    """No module of the package other than ops.py (which picks the binding) and _ctypes_ops.py (which is one) mentions `ctypes_hip`: a
    facade calls `ops.hip.<name>` and nothing else."""
    pkg = os.path.join(ROOT, "diffmusic_amd")
    seen = 0
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                seen += 1
                path = os.path.join(dp, f)
                if os.path.relpath(path, pkg) not in ("ops.py", "_ctypes_ops.py"):
                    assert "ctypes_hip" not in open(path).read(), path
    assert seen >= 10
