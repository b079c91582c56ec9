"""CPU: the C ABI of libngp_metrics.so (header, exports, ctypes, build entry, the window's literals, the tile constants, host-side
argument checks), the numpy restatement the GPU tests compare against (tests/metrics_reference.py) held to known answers, to the
float64 definition and to the torch statement, and the accumulation arithmetic of the two metric classes."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import metrics_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngp_metrics.h")
OTHERS = ("ngp_hip.h", "ngp_mesh.h", "ngp_meshfilter.h", "ngp_meshcull.h", "ngp_meshsimplify.h", "ngp_meshtsdf.h", "ngp_meshsmooth.h",
          "ngp_meshtex.h")
F = np.float32


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (\w+)", out))


def _define(name):
    m = re.search(r"^#define\s+%s\s+(-?\w+)" % name, open(HEADER).read(), flags=re.M)
    return int(m.group(1))


# ---- 1. the C ABI


def test_header_compiles_as_c99_alone_and_with_the_other_eight():
    inc = lambda names: "".join('#include "%s"\n' % n for n in names)
    use = "static const float g[NGP_METRICS_WINDOW_TAPS] = NGP_METRICS_WINDOW;\nint main(void) { return (int)g[0] + NGP_EINVAL + NGP_ERANGE; }\n"
    for src in ('#include "ngp_metrics.h"\n' + use, inc(OTHERS + ("ngp_metrics.h",)) + use, inc(("ngp_metrics.h",) + OTHERS[::-1]) + use):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            "-x", "c", "-"], input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == {"stddef.h", "stdint.h"}
    assert "#ifndef NGP_EINVAL" in text and "#ifndef NGP_ERANGE" in text and "THE RULE" in text


def test_library_exports_exactly_its_header_and_ctypes_agrees():
    from ngp_pl_amd import _abi, _metrics_lib
    protos = _abi.parse(HEADER)
    assert set(protos) == {"ngp_metrics_" + n for n in ("abi_version", "build_arch", "tile", "workspace_bytes", "sq_error", "ssim")}
    assert _exports(_metrics_lib.LIB_PATH) == set(protos)
    assert set(_metrics_lib.exported_symbols()) == set(protos)
    lib = _metrics_lib.lib()
    assert lib.ngp_metrics_abi_version() == 1 == _metrics_lib.ABI_VERSION and lib.ngp_metrics_build_arch() == b"gfx950"
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in _metrics_lib._PROTOS.items()) if m]
    assert not problems, "\n".join(problems)
    for name, pr in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and _abi.ctypes_agrees(list(f.argtypes), pr) is None, name
        assert f.restype is {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[pr.ret], name


def test_the_ninth_library_shares_no_symbol_with_the_other_eight():
    from ngp_pl_amd import (_abi, _lib, _mesh_lib, _meshcull_lib, _meshfilter_lib, _meshsimplify_lib, _meshsmooth_lib, _meshtex_lib,
                            _meshtsdf_lib, _metrics_lib)
    mods = (_lib, _mesh_lib, _meshfilter_lib, _meshcull_lib, _meshsimplify_lib, _meshtsdf_lib, _meshsmooth_lib, _meshtex_lib, _metrics_lib)
    assert len({m.LIB_PATH for m in mods}) == 9
    exports = [_exports(m.LIB_PATH) for m in mods]
    own, others = exports[-1], set().union(*exports[:-1])
    assert own and not own & others
    assert not [s for s in others if s.startswith("ngp_metrics")] and not [s for s in own if not s.startswith("ngp_metrics_")]
    declared_elsewhere = set(_abi.parse_all())
    for h in OTHERS[1:]:
        declared_elsewhere |= set(_abi.parse(os.path.join(ROOT, "include", h)))
    assert not set(_abi.parse(HEADER)) & declared_elsewhere


def test_build_links_the_ninth_library_with_contraction_off():
    from ngp_pl_amd import _metrics_lib, build
    assert build.METRICS_LIB == _metrics_lib.LIB_PATH and build.METRICS_CFLAGS == ["-ffp-contract=off"]
    assert build.METRICS_SOURCES == [os.path.join("metrics", "metrics.hip")]
    assert all(os.path.exists(os.path.join(build.CSRC, s)) for s in build.METRICS_SOURCES + build.METRICS_HEADERS)
    blob = open(_metrics_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob
    for kernel in (b"ssim_tile", b"sq_tile", b"finish"):
        assert kernel in blob


def test_window_literals_equal_the_formula():
    text = open(HEADER).read()
    body = re.search(r"#define NGP_METRICS_WINDOW \\\n(.*?)\}", text, flags=re.S).group(1)
    lits = re.findall(r"0x[0-9a-fA-F.]+p[-+]?\d+f", body)
    assert len(lits) == 11
    got = np.array([float.fromhex(x[:-1]) for x in lits])
    want = R.window()
    assert got.astype(F).tobytes() == want.tobytes() and np.array_equal(got, want.astype(np.float64))        # exact f32 values, mirrored
    assert np.array_equal(want, want[::-1])
    for g, ref in zip(want[:6], (0.0010283801, 0.0075987582, 0.036000773, 0.10936069, 0.21300554, 0.26601171)):
        assert abs(float(g) - ref) < 5e-8 * max(ref, 0.01)
    assert abs(float(want.astype(np.float64).sum()) - 0.9999999986) < 1e-10


def test_tile_and_constants_equal_the_headers():
    from ngp_pl_amd import _metrics_lib as L
    w, h = C.c_int(-1), C.c_int(-1)
    assert L.lib().ngp_metrics_tile(C.byref(w), C.byref(h)) == 0
    assert (w.value, h.value) == (L.TILE_W, L.TILE_H) == (_define("NGP_METRICS_TILE_W"), _define("NGP_METRICS_TILE_H"))
    assert L.TILE_W >= 64
    assert L.lib().ngp_metrics_tile(None, C.byref(h)) == -1
    assert (L.HWC, L.CHW) == (_define("NGP_METRICS_HWC"), _define("NGP_METRICS_CHW"))
    assert (L.SQ_THREADS, L.SQ_MAX_BLOCKS) == (_define("NGP_METRICS_SQ_THREADS"), _define("NGP_METRICS_SQ_MAX_BLOCKS"))
    assert (L.MAX_CHANNELS, L.MAX_SIDE, L.WINDOW_TAPS) == (_define("NGP_METRICS_MAX_CHANNELS"), _define("NGP_METRICS_MAX_SIDE"),
                                                           _define("NGP_METRICS_WINDOW_TAPS")) == (4, 16384, R.TAPS)


def test_workspace_bytes_and_host_side_refusals():
    """Nothing below reaches a launch: every call is refused on the host (the pointers are never looked through)."""
    from ngp_pl_amd import _metrics_lib as L
    lib = L.lib()
    wb = lib.ngp_metrics_workspace_bytes
    tiles = lambda h, w: -(-(h - 10) // L.TILE_H) * -(-(w - 10) // L.TILE_W) if h > 10 and w > 10 else 0
    sqb = lambda c, h, w: min(-(-(c * h * w) // L.SQ_THREADS), L.SQ_MAX_BLOCKS)
    for n, c, h, w in ((1, 1, 11, 11), (3, 3, 35, 139), (1, 4, 800, 800), (200, 3, 800, 800), (1, 1, 1, 1), (2, 3, 5, 300), (1, 1, 16384, 16384)):
        assert wb(n, c, h, w) == 16 * n * max(tiles(h, w), sqb(c, h, w)), (n, c, h, w)
    for bad in ((0, 3, 20, 20), (1, 0, 20, 20), (1, 5, 20, 20), (1, 3, 0, 20), (1, 3, 20, 16385), (1 << 31, 1, 11, 11)):
        assert wb(*bad) == 0, bad
    one = 0x1000                                      # a non-null, 8-byte aligned address that is never dereferenced on the host
    ok = dict(pred=one, target=one, mask=None, n=1, c=3, h=20, w=20, layout=0, dr=1.0, ws=one, wsb=1 << 20, s=one, k=one, m=None)

    def ssim(**kw):
        a = dict(ok, **kw)
        return lib.ngp_metrics_ssim(a["pred"], a["target"], a["mask"], a["n"], a["c"], a["h"], a["w"], a["layout"], a["dr"], a["ws"], a["wsb"],
                                    a["s"], a["k"], a["m"], None)

    def sq(**kw):
        a = dict(ok, **kw)
        return lib.ngp_metrics_sq_error(a["pred"], a["target"], a["mask"], a["n"], a["c"], a["h"], a["w"], a["layout"], a["ws"], a["wsb"],
                                        a["s"], a["k"], None)

    need = wb(1, 3, 20, 20)
    for kw in (dict(pred=None), dict(target=None), dict(ws=None), dict(s=None), dict(k=None), dict(n=0), dict(c=0), dict(c=5), dict(h=10),
               dict(w=10), dict(layout=2), dict(layout=-1), dict(wsb=need - 1), dict(ws=one + 4), dict(dr=0.0), dict(dr=-1.0),
               dict(dr=float("nan")), dict(dr=float("inf"))):
        assert ssim(**kw) == -1, kw
    for kw in (dict(pred=None), dict(target=None), dict(ws=None), dict(s=None), dict(k=None), dict(n=0), dict(c=5), dict(h=0), dict(w=0),
               dict(layout=2), dict(wsb=need - 1)):
        assert sq(**kw) == -1, kw
    for kw in (dict(h=16385), dict(w=16385), dict(n=1 << 31)):
        assert ssim(**kw) == -5 and sq(**kw) == -5, kw


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    from ngp_pl_amd import metrics
    a = torch.zeros(1, 20, 20, 3)
    for fn in (metrics.sq_error, metrics.psnr, metrics.ssim):
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(a, a)
    with pytest.raises(ValueError):
        metrics.ssim(a, a, layout="nhwc")
    with pytest.raises(ValueError):
        metrics.ssim(a, a, data_range=0.0)
    assert not hasattr(metrics, "LearnedPerceptualImagePatchSimilarity") and "LPIPS" in metrics.__doc__


# ---- 2. the restatement against known answers


def test_identical_images_give_exactly_one():
    for kind in ("noise", "smooth", "quantised", "range4"):
        p, _, dr = R.images(kind, 2, 23, 30, 3)
        m, sums, counts = R.ssim_f32(p, p.copy(), dr)
        assert m.dtype == F and m.shape == (2, 13, 20, 3)
        assert np.array_equal(m.view(np.int32), np.full(m.shape, 0x3F800000, np.int32))      # numerator and denominator are one number
        assert counts == [13 * 20 * 3] * 2 and sums == [float(c) for c in counts]


def test_constant_images_against_the_closed_form():
    for a, b, dr in ((0.25, 0.75, 1.0), (1.0, 0.0, 1.0), (3.0, 1.5, 4.0), (0.5, 0.5, 1.0)):
        p, t = np.full((1, 15, 17, 2), a, F), np.full((1, 15, 17, 2), b, F)
        m, sums, counts = R.ssim_f32(p, t, dr)
        c1 = (0.01 * dr) ** 2
        want = (2 * a * b + c1) / (a * a + b * b + c1)            # the variances vanish: the second factor is c2 / c2
        # The first factor carries a few f32 roundings of values near 1: 2e-6.  The second is (2 spt + c2) / (spp + stt + c2) with
        # variances that are rounding residue: each of pp, mp * mp, ... comes out of at most 24 roundings of a value <= max(a, b)^2,
        # so the four residues together shift the factor by at most 4 * 24 * 2^-24 * max(a, b)^2 / c2.
        c2 = (0.03 * dr) ** 2
        tol = 2e-6 + 4 * 24 * 2.0 ** -24 * max(a, b) ** 2 / c2
        assert np.abs(m.astype(np.float64) - want).max() < tol, (a, b)
        assert counts == [5 * 7 * 2] and abs(sums[0] / counts[0] - want) < tol


def test_masks_select_windows_by_their_centre_pixel():
    p, t, dr = R.images("noise", 2, 14, 16, 1)
    mask = np.zeros((2, 14, 16), np.uint8)
    mask[0, 5, 5] = 1          # window (0, 0) of image 0
    mask[0, 4, 8] = 1          # within 5 pixels of the border: no window has its centre there
    mask[1, 8, 10] = 7         # window (3, 5) of image 1
    m, sums, counts = R.ssim_f32(p, t, dr, mask)
    assert counts == [1, 1] and sums == [float(m[0, 0, 0, 0]), float(m[1, 3, 5, 0])]
    se, k = R.sq_error_f32(p, t, mask)
    assert k == [2, 1]
    d = (p - t).astype(F)
    assert se[1] == float(F(d[1, 8, 10, 0] * d[1, 8, 10, 0]))
    assert math.isnan(R.psnr(0.0, 0)) and R.psnr(0.0, 5) == float("inf") and math.isnan(R.mean(0.0, 0))
    assert abs(R.psnr(0.5, 50, 1.0) - 20.0) < 1e-12


# ---- 3. the f32 rule against the float64 definition and against the torch statement, on the inputs of the GPU tests

# The largest |f32 rule - other| over tests.metrics_reference.cases(64, 12) per input class, as measured with this file's code; the
# test asserts four times that (the inputs are seeded and the classes differ by orders of magnitude).  "flat" is the worst: the
# variances cancel against c2 = 9e-4.  "white" measured 0 against both; it gets the f32 bound of the ~25 operations behind a value
# of 1 instead (25 * 2^-24 = 1.5e-6 -> 2e-6), since a convolution may add its taps in another order.
MEASURED_VS_F64 = {"noise": 2.38e-6, "smooth": 5.49e-5, "flat": 1.87e-4, "quantised": 4.99e-5, "white": 0.0, "range4": 1.95e-6}
MEASURED_VS_TORCH = {"noise": 6.62e-6, "smooth": 1.42e-4, "flat": 3.97e-4, "quantised": 1.87e-4, "white": 0.0, "range4": 5.73e-6}
WHITE_BOUND = 2e-6


def test_cases_cover_every_size_class_channel_count_and_layout():
    from ngp_pl_amd import _metrics_lib as L
    cs = R.cases(L.TILE_W, L.TILE_H)
    assert {c[2] for c in cs} == {11, 12, 21, L.TILE_H + 9, L.TILE_H + 10, L.TILE_H + 11, 2 * L.TILE_H + 11}
    assert {c[3] for c in cs} == {11, 12, 21, L.TILE_W + 9, L.TILE_W + 10, L.TILE_W + 11, 2 * L.TILE_W + 11}
    assert {c[0] for c in cs} == set(R.CLASSES) and {c[1] for c in cs} == {1, 3} and {c[4] for c in cs} == {1, 3, 4}
    assert {(c[0], c[5]) for c in cs} == {(k, l) for k in R.CLASSES for l in ("hwc", "chw")}
    assert {(c[0], c[4]) for c in cs} == {(k, l) for k in R.CLASSES for l in (1, 3, 4)} and {(c[0], c[1]) for c in cs} == {(k, l) for k in R.CLASSES for l in (1, 3)}
    assert {(c[4], c[5]) for c in cs} == {(k, l) for k in (1, 3, 4) for l in ("hwc", "chw")}


def test_f32_rule_against_the_float64_definition_and_the_torch_statement():
    from ngp_pl_amd import _metrics_lib as L
    worst64, worst_t = dict.fromkeys(R.CLASSES, 0.0), dict.fromkeys(R.CLASSES, 0.0)
    for case in R.cases(L.TILE_W, L.TILE_H):
        p, t, dr = R.case_images(case)
        m, _, _ = R.ssim_f32(p, t, dr, None, case[5])
        a, b = R.ssim_f64(p, t, dr, case[5]), R.ssim_torch(p, t, dr, case[5])
        assert m.shape == a.shape == b.shape
        worst64[case[0]] = max(worst64[case[0]], float(np.abs(m - a).max()))
        worst_t[case[0]] = max(worst_t[case[0]], float(np.abs(m - b).max()))
    print("f32 rule vs float64 definition:", worst64)
    print("f32 rule vs torch statement:   ", worst_t)
    for kind in R.CLASSES:
        assert worst64[kind] <= max(4 * MEASURED_VS_F64[kind], WHITE_BOUND if kind == "white" else 0.0), (kind, worst64[kind])
        assert worst_t[kind] <= max(4 * MEASURED_VS_TORCH[kind], WHITE_BOUND if kind == "white" else 0.0), (kind, worst_t[kind])


def test_squared_error_restatement_against_float64():
    p, t, _ = R.images("noise", 2, 13, 9, 3)
    mask = (np.random.RandomState(3).rand(2, 13, 9) < 0.5).astype(np.uint8)
    for layout in ("hwc", "chw"):
        q, u = (p, t) if layout == "hwc" else (np.moveaxis(p, -1, 1).copy(), np.moveaxis(t, -1, 1).copy())
        for m in (None, mask):
            (s32, k32), (s64, k64) = R.sq_error_f32(q, u, m, layout), R.sq_error_f64(q, u, m, layout)
            assert k32 == k64 == ([13 * 9 * 3] * 2 if m is None else [int(mask[i].sum()) * 3 for i in range(2)])
            for a, b, k in zip(s32, s64, k32):
                assert abs(a - b) <= k * 2.0 ** -23        # d * d rounds once in f32, |d * d| <= 1


# ---- 4. the classes' accumulation, the two native functions replaced by the restatement


def _patch(monkeypatch):
    from ngp_pl_amd import metrics

    def sq_error(pred, target, mask=None, layout="hwc"):
        s, k = R.sq_error_f32(pred.numpy(), target.numpy(), None if mask is None else mask.numpy(), layout)
        return torch.tensor(s, dtype=torch.float64), torch.tensor(k, dtype=torch.int64)

    def ssim(pred, target, data_range=1.0, mask=None, layout="hwc", return_map=False):
        _, s, k = R.ssim_f32(pred.numpy(), target.numpy(), data_range, None if mask is None else mask.numpy(), layout)
        return torch.tensor(s, dtype=torch.float64) / torch.tensor(k, dtype=torch.float64)

    monkeypatch.setattr(metrics, "sq_error", sq_error)
    monkeypatch.setattr(metrics, "ssim", ssim)
    return metrics


def test_psnr_class_accumulates_squared_error_and_count(monkeypatch):
    metrics = _patch(monkeypatch)
    g = np.random.RandomState(0)
    a1, b1 = g.rand(2, 3, 12, 13).astype(F), g.rand(2, 3, 12, 13).astype(F)
    a2, b2 = g.rand(1, 3, 20, 11).astype(F), g.rand(1, 3, 20, 11).astype(F)
    m = metrics.PeakSignalNoiseRatio(data_range=1)
    first = m(torch.from_numpy(a1), torch.from_numpy(b1))
    m.update(torch.from_numpy(a2), torch.from_numpy(b2))
    e1 = ((a1 - b1).astype(F) ** 2).astype(np.float64)
    e2 = ((a2 - b2).astype(F) ** 2).astype(np.float64)
    assert abs(first.item() - R.psnr(math.fsum(e1.ravel()), e1.size)) < 1e-9
    total, count = math.fsum(e1.ravel()) + math.fsum(e2.ravel()), e1.size + e2.size
    assert int(m.total) == count and abs(m.compute().item() - R.psnr(total, count)) < 1e-9
    m.reset()
    with pytest.raises(RuntimeError):
        m.compute()
    same = metrics.PeakSignalNoiseRatio(data_range=2.0)
    same.update(torch.from_numpy(a2), torch.from_numpy(a2))
    assert same.compute().item() == float("inf")
    odd = metrics.PeakSignalNoiseRatio()                          # any shape: a vector of 7 elements
    odd.update(torch.from_numpy(a1.ravel()[:7].copy()), torch.from_numpy(b1.ravel()[:7].copy()))
    assert int(odd.total) == 7 and abs(odd.compute().item() - R.psnr(math.fsum(e1.ravel()[:7]), 7)) < 1e-9


def test_ssim_class_averages_the_per_image_scores(monkeypatch):
    metrics = _patch(monkeypatch)
    g = np.random.RandomState(1)
    a1, b1 = g.rand(2, 3, 12, 13).astype(F), g.rand(2, 3, 12, 13).astype(F)
    a2, b2 = g.rand(1, 3, 20, 11).astype(F), g.rand(1, 3, 20, 11).astype(F)
    m = metrics.StructuralSimilarityIndexMeasure(data_range=1)
    first = m(torch.from_numpy(a1), torch.from_numpy(b1))
    m.update(torch.from_numpy(a2), torch.from_numpy(b2))
    scores = []
    for a, b in ((a1, b1), (a2, b2)):
        _, s, k = R.ssim_f32(a, b, 1.0, None, "chw")
        scores += [x / y for x, y in zip(s, k)]
    assert abs(first.item() - sum(scores[:2]) / 2) < 1e-12
    assert m.total == 3 and abs(m.compute().item() - sum(scores) / 3) < 1e-12
    m.reset()
    with pytest.raises(RuntimeError):
        m.compute()
    with pytest.raises(ValueError):
        m.update(torch.zeros(3, 12, 13), torch.zeros(3, 12, 13))
