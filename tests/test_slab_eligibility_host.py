"""CPU: which launches the tap-stationary 320 x 256 tile (tile_cfg 20 / 21 / 22, csrc/gemm_tile.h) may take -- the C predicate
`dmx_gemm_slab_eligible` against a plain-Python restatement over a table of descriptors: one refused descriptor per rule, and the
36 wide-stage HiFi-GAN launches of the benchmark step (profiles/r05_gemm_shapes.csv), each accepted."""
import csv
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALO = 64
EXCLUDED = 128 | 4096 | 8192 | 16384 | 32768 | 65536 | 131072     # F32OUT, SOFTBWD, GEGLU, LNFOLD, ROWSTATS, GNSTATS, GNBWD


def _lib():
    from diffmusic_amd import _lib as L
    from diffmusic_amd.build import build_library
    build_library()
    h = C.CDLL(L.LIB_PATH)
    h.dmx_gemm_slab_eligible.restype = C.c_int
    h.dmx_gemm_slab_eligible.argtypes = [C.c_void_p, C.c_size_t]
    return L, h


def _conv(L, B=8, T=5001, Ci=512, Co=512, k=3, dil=1, flags=1 | 32 | 256, **kw):
    """descriptor of a 'same' 1-D convolution as csrc/layers.hip builds it (no pointers: the predicate is host arithmetic)"""
    d = L.GemmDesc()
    d.Z = d.Zi = 1
    d.sy = d.sx = d.osy = d.osx = 1
    d.alpha = 1.0
    pad = (k - 1) * dil // 2
    d.M, d.N, d.K, d.ldw = B * T, Co, k * Ci, k * Ci
    d.Hi, d.Wi, d.Ci, d.lda = 1, T, Ci, Ci
    d.Hq, d.Wq, d.ntaps = 1, T, k
    d.Ho, d.Wo = 1, T
    d.ldc = d.ldr = d.ldx = d.ldc2 = Co
    d.flags = flags
    for t in range(k):
        d.tdx[t] = t * dil - pad
    for key, v in kw.items():
        if key in ("tdy", "tdx"):
            for i, t in enumerate(v):
                getattr(d, key)[i] = t
        else:
            setattr(d, key, v)
    return d


def _glds_ok(d):
    imgs = -(-d.M // (d.Hq * d.Wq)) if d.Hq * d.Wq > 0 else 1
    in_elems = (imgs * d.Hi * d.Wi if (d.Hi > 1 or d.ntaps > 1) else d.M) * d.lda
    return in_elems < 2 ** 29 and d.M * d.lda < 2 ** 29 and (d.N + 512) * d.ldw < 2 ** 29


def _restated(d):
    tdx, tdy = list(d.tdx)[:max(d.ntaps, 0)], list(d.tdy)[:max(d.ntaps, 0)]
    return (d.Hi == 1 and d.Hq == 1 and d.sx == 1 and 2 <= d.ntaps <= 16 and d.Ci > 0 and d.Ci % 64 == 0 and d.N > 0 and d.N % 256 == 0
            and d.Wq > 0 and d.M % d.Wq == 0 and d.ksplit <= 1 and all(t == 0 for t in tdy) and max(tdx) - min(tdx) <= HALO
            and not (d.flags & EXCLUDED) and (d.ldc | d.ldr | d.ldx | d.ldc2) % 8 == 0 and _glds_ok(d))


def _refused(L):
    two_d = _conv(L, k=9, Ci=128, Co=256, Hi=37, Hq=37, tdy=[t // 3 - 1 for t in range(9)], tdx=[t % 3 - 1 for t in range(9)])
    two_d.M, two_d.Wi, two_d.Wq = 2 * 37 * 16, 16, 16
    return {
        "2-D": two_d,
        "2-D taps over one input row": _conv(L, tdy=[0, 1, 0]),
        "strided": _conv(L, sx=2),
        "Ci = 40": _conv(L, Ci=40),
        "span 65": _conv(L, k=2, tdx=[-32, 33]),
        "N = 128": _conv(L, Co=128),
        "ntaps = 1": _conv(L, k=1),
        "fp32 output": _conv(L, flags=128),
        "GroupNorm statistics": _conv(L, flags=1 | 65536),
        "split-K slice": _conv(L, ksplit=2),
        "rows that are no whole images": _conv(L, M=8 * 5001 - 1),
        "operand span past the 32-bit offsets": _conv(L, B=300, T=8000, Ci=256, Co=256),
    }


def _wide_stage_rows():
    rows = []
    with open(os.path.join(ROOT, "profiles", "r05_gemm_shapes.csv")) as fh:
        for r in csv.DictReader(fh):
            r = {k: int(v) for k, v in r.items() if k not in ("ms", "tflops")}
            if r["cfg"] == 7 and r["taps"] in (3, 7, 11) and r["flags"] >= 256:       # (the resblock convolutions of the C = 512 / 256 stages)
                rows.append(r)
    return rows


def test_the_restatement_knows_the_boundaries():
    L, _ = _lib()
    assert _restated(_conv(L)) and _restated(_conv(L, k=2, tdx=[-32, 32])) and _restated(_conv(L, k=11, dil=5, Ci=256, Co=256))
    assert len(_wide_stage_rows()) == 36


@pytest.mark.parametrize("name", ["2-D", "2-D taps over one input row", "strided", "Ci = 40", "span 65", "N = 128", "ntaps = 1", "fp32 output",
                                  "GroupNorm statistics", "split-K slice", "rows that are no whole images",
                                  "operand span past the 32-bit offsets"])
def test_each_rule_refuses(name):
    L, h = _lib()
    d = _refused(L)[name]
    assert not _restated(d), name
    assert h.dmx_gemm_slab_eligible(C.byref(d), C.sizeof(d)) == 0, name


def test_wide_stage_descriptors_are_accepted():
    L, h = _lib()
    for r in _wide_stage_rows():
        for dil in (1, 3, 5):
            for flip in (False, True):
                k, Ci = r["taps"], r["K"] // r["taps"]
                pad = (k - 1) * dil // 2
                tdx = [(pad - t * dil) if flip else (t * dil - pad) for t in range(k)]
                d = _conv(L, B=8, T=r["M"] // 8, Ci=Ci, Co=r["N"], k=k, dil=dil, flags=r["flags"], tdx=tdx)
                assert (d.M, d.N, d.K) == (r["M"], r["N"], r["K"])
                assert _restated(d), (r, dil)
                assert h.dmx_gemm_slab_eligible(C.byref(d), C.sizeof(d)) == 1, (r, dil)


def test_predicate_and_restatement_agree_on_a_sweep():
    L, h = _lib()
    n = 0
    for k in (1, 2, 3, 7, 11, 16):
        for dil in (1, 3, 5, 7):
            for Ci in (32, 64, 192, 200):
                for Co in (128, 256, 384, 512):
                    for sx in (1, 2):
                        d = _conv(L, B=3, T=700, Ci=Ci, Co=Co, k=k, dil=dil, sx=sx)
                        assert h.dmx_gemm_slab_eligible(C.byref(d), C.sizeof(d)) == int(_restated(d)), (k, dil, Ci, Co, sx)
                        n += 1
    assert n == 768


def test_size_mismatch_is_an_error():
    L, h = _lib()
    d = _conv(L)
    assert h.dmx_gemm_slab_eligible(C.byref(d), C.sizeof(d) - 8) < 0
