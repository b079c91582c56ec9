"""CPU: the C ABI of libngp_meshdist.so (header, exports, ctypes, build entry, constants, host-side argument checks), the numpy
restatement the GPU tests compare against (tests/mesh_distance_reference.py) held to known answers and to the float64 definition,
and the PLY reader against the writer."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import mesh_distance_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngp_meshdist.h")
OTHERS = ("ngp_hip.h", "ngp_mesh.h", "ngp_meshfilter.h", "ngp_meshcull.h", "ngp_meshsimplify.h", "ngp_meshtsdf.h", "ngp_meshsmooth.h",
          "ngp_meshtex.h", "ngp_metrics.h")
F = np.float32
NAMES = ("abi_version", "build_arch", "slack", "sample_workspace_bytes", "sample_count", "sample_emit", "grid_workspace_bytes",
         "grid_count", "grid_fill", "query", "stats_workspace_bytes", "stats")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (\w+)", out))


def _define(name):
    m = re.search(r"^#define\s+%s\s+(-?\w+)" % name, open(HEADER).read(), flags=re.M)
    return int(m.group(1))


# ---- 1. the C ABI


def test_header_compiles_as_c99_alone_and_with_the_other_nine():
    inc = lambda names: "".join('#include "%s"\n' % n for n in names)
    use = "int main(void) { return NGP_MESHDIST_K_MAX + NGP_EINVAL + NGP_ERANGE; }\n"
    for src in ('#include "ngp_meshdist.h"\n' + use, inc(OTHERS + ("ngp_meshdist.h",)) + use, inc(("ngp_meshdist.h",) + OTHERS[::-1]) + use):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            "-x", "c", "-"], input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == {"stddef.h", "stdint.h"}
    assert "#ifndef NGP_EINVAL" in text and "#ifndef NGP_ERANGE" in text and "THE RULE" in text and "SLACK." in text


def test_library_exports_exactly_its_header_and_ctypes_agrees():
    from ngp_pl_amd import _abi, _meshdist_lib
    protos = _abi.parse(HEADER)
    assert set(protos) == {"ngp_meshdist_" + n for n in NAMES}
    assert _exports(_meshdist_lib.LIB_PATH) == set(protos)
    assert set(_meshdist_lib.exported_symbols()) == set(protos)
    lib = _meshdist_lib.lib()
    assert lib.ngp_meshdist_abi_version() == 1 == _meshdist_lib.ABI_VERSION and lib.ngp_meshdist_build_arch() == b"gfx950"
    tables = dict(_meshdist_lib._PROTOS, **_meshdist_lib._SIZES)
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in tables.items()) if m]
    assert not problems, "\n".join(problems)
    for name, pr in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and _abi.ctypes_agrees(list(f.argtypes), pr) is None, name
        assert f.restype is {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[pr.ret], name


def test_the_tenth_library_shares_no_symbol_with_the_other_nine():
    from ngp_pl_amd import (_abi, _lib, _mesh_lib, _meshcull_lib, _meshdist_lib, _meshfilter_lib, _meshsimplify_lib, _meshsmooth_lib,
                            _meshtex_lib, _meshtsdf_lib, _metrics_lib)
    mods = (_lib, _mesh_lib, _meshfilter_lib, _meshcull_lib, _meshsimplify_lib, _meshtsdf_lib, _meshsmooth_lib, _meshtex_lib, _metrics_lib,
            _meshdist_lib)
    assert len({m.LIB_PATH for m in mods}) == 10
    exports = [_exports(m.LIB_PATH) for m in mods]
    own, others = exports[-1], set().union(*exports[:-1])
    assert own and not own & others
    assert not [s for s in others if s.startswith("ngp_meshdist")] and not [s for s in own if not s.startswith("ngp_meshdist_")]
    declared_elsewhere = set(_abi.parse_all())
    for h in OTHERS[1:]:
        declared_elsewhere |= set(_abi.parse(os.path.join(ROOT, "include", h)))
    assert not set(_abi.parse(HEADER)) & declared_elsewhere


def test_build_links_the_tenth_library_with_contraction_off():
    from ngp_pl_amd import _meshdist_lib, build
    assert build.MESHDIST_LIB == _meshdist_lib.LIB_PATH and build.MESHDIST_CFLAGS == ["-ffp-contract=off"]
    assert build.MESHDIST_SOURCES == [os.path.join("meshdist", "meshdist.hip")]
    assert all(os.path.exists(os.path.join(build.CSRC, s)) for s in build.MESHDIST_SOURCES + build.MESHDIST_HEADERS)
    assert "-fhip-fp32-correctly-rounded-divide-sqrt" in build.CFLAGS
    blob = open(_meshdist_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob
    for kernel in (b"face_counts", b"emit_samples", b"bin_faces", b"query", b"stats_finish", b"scan_block_sums"):
        assert kernel in blob


def test_constants_equal_the_headers():
    from ngp_pl_amd import _meshdist_lib as L
    for name in ("K_MAX", "MAX_AXIS", "MAX_CELLS", "MAX_THRESHOLDS", "SLACK_ULPS", "MIN_CELL_SLACKS", "SCAN_BLOCK", "STATS_MAX_BLOCKS",
                 "STATS_OUTPUTS"):
        assert getattr(L, name) == _define("NGP_MESHDIST_" + name), name
    assert (L.K_MAX, L.MAX_AXIS, L.MAX_CELLS, L.MAX_THRESHOLDS) == (64, 1024, 2 ** 30, 8) and R.K_MAX == L.K_MAX and R.SLACK_ULPS == L.SLACK_ULPS
    # the slack is the multiple of 2^-23 x the magnitude the header derives, and more than its bound of 24.5 asks
    s, m = L.slack((-3.0, 0.0, 1.0), 0.5, (4, 2, 8))           # M_grid = max(|-3|, |-3 + 2|, |0 + 1|, |1 + 4|) = 5
    assert s == float(R.slack(5.0)) == 64 * 2.0 ** -23 * 5.0 and m == 8 * s
    assert L.SLACK_ULPS > 24.5 and 2 * R.lower_error(1.0) / 2.0 ** -23 == 33.0


def test_workspace_bytes_and_host_side_refusals():
    """Nothing below reaches a launch: every call is refused on the host (the device pointers are never looked through)."""
    from ngp_pl_amd import _meshdist_lib as L
    lib = L.lib()
    blocks = lambda n: -(-n // L.SCAN_BLOCK)
    for n in (1, 2047, 2048, 2049, 10 ** 6):
        assert lib.ngp_meshdist_sample_workspace_bytes(n) == 8 * (n + 1) + 8 * blocks(n) + (4 * n + 7) // 8 * 8, n
        assert lib.ngp_meshdist_stats_workspace_bytes(n) == 14 * 8 * min(-(-n // 256), 512), n
    for bad in (0, -1, 2 ** 31):
        assert lib.ngp_meshdist_sample_workspace_bytes(bad) == 0 and lib.ngp_meshdist_stats_workspace_bytes(bad) == 0
    for dims in ((1, 1, 1), (2, 3, 5), (1024, 1024, 1024), (52, 52, 52)):
        n = dims[0] * dims[1] * dims[2]
        assert lib.ngp_meshdist_grid_workspace_bytes(*dims) == 8 * blocks(n) + 4 * (n + 1) + 4 * n
    for dims in ((0, 1, 1), (1, 1025, 1), (1, 1, -1)):
        assert lib.ngp_meshdist_grid_workspace_bytes(*dims) == 0, dims

    one = 0x1000                                      # a non-null, 8-byte aligned address that is never dereferenced on the host
    big = 1 << 40
    origin, th = L.floats((0, 0, 0)), L.floats((0.1, 0.2))
    ok = dict(v=one, f=one, nv=10, nf=10, sp=0.5, ws=one, wsb=big, tot=one, ns=5, pts=one, wts=one, ids=one, o=origin, cell=0.25, nx=4, ny=4,
              nz=4, ne=5, ent=one, p=one, np=3, md=1.0, d2=one, face=one, n=7, th=th, nt=2, out=one)

    def sample_count(**kw):
        a = dict(ok, **kw)
        return lib.ngp_meshdist_sample_count(a["v"], a["f"], a["nv"], a["nf"], a["sp"], a["ws"], a["wsb"], a["tot"], None)

    def sample_emit(**kw):
        a = dict(ok, **kw)
        return lib.ngp_meshdist_sample_emit(a["v"], a["f"], a["nv"], a["nf"], a["sp"], a["ws"], a["wsb"], a["ns"], a["pts"], a["wts"], a["ids"], None)

    def grid_count(**kw):
        a = dict(ok, **kw)
        return lib.ngp_meshdist_grid_count(a["v"], a["f"], a["nv"], a["nf"], a["o"], a["cell"], a["nx"], a["ny"], a["nz"], a["ws"], a["wsb"],
                                           a["tot"], None)

    def grid_fill(**kw):
        a = dict(ok, **kw)
        return lib.ngp_meshdist_grid_fill(a["v"], a["f"], a["nv"], a["nf"], a["o"], a["cell"], a["nx"], a["ny"], a["nz"], a["ws"], a["wsb"],
                                          a["ne"], a["ent"], None)

    def query(**kw):
        a = dict(ok, **kw)
        return lib.ngp_meshdist_query(a["p"], a["np"], a["v"], a["f"], a["nv"], a["nf"], a["o"], a["cell"], a["nx"], a["ny"], a["nz"], a["md"],
                                      a["ws"], a["wsb"], a["ent"], a["ne"], a["d2"], a["face"], None, None, None)

    def stats(**kw):
        a = dict(ok, **kw)
        return lib.ngp_meshdist_stats(a["d2"], a["face"], a["wts"], a["n"], a["th"], a["nt"], a["ws"], a["wsb"], a["out"], None)

    need = lib.ngp_meshdist_sample_workspace_bytes(10)
    sampler = (dict(v=None), dict(f=None), dict(ws=None), dict(nv=-1), dict(nf=-1), dict(sp=0.0), dict(sp=-1.0), dict(sp=float("nan")),
               dict(sp=float("inf")), dict(wsb=need - 1), dict(ws=one + 4))
    for kw in sampler + (dict(tot=None),):
        assert sample_count(**kw) == -1, kw
    for kw in sampler + (dict(ns=-1), dict(pts=None), dict(wts=None), dict(ids=None)):
        assert sample_emit(**kw) == -1, kw
    for kw in (dict(nv=2 ** 31), dict(nf=2 ** 31)):
        assert sample_count(**kw) == -5 and sample_emit(**kw) == -5, kw
    assert sample_emit(ns=2 ** 31) == -5

    gneed = lib.ngp_meshdist_grid_workspace_bytes(4, 4, 4)
    small = L.slack((0, 0, 0), 0.25, (4, 4, 4))[1]     # the smallest cell the grid of magnitude 1 takes: 2^-14
    assert small == 2.0 ** -14
    # a cell below the documented ratio: 1000 at the origin's magnitude asks for cell >= 2^-14 * (1000 + 4 cell)
    far = L.floats((1000.0, 0.0, 0.0))
    grid = (dict(v=None), dict(f=None), dict(o=None), dict(ws=None), dict(nv=-1), dict(nf=-1), dict(nx=0), dict(ny=1025), dict(nz=-3),
            dict(nx=1024, ny=1024, nz=1025), dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")),
            dict(o=L.floats((float("nan"), 0, 0))), dict(o=far, cell=0.05), dict(o=far, cell=0.06), dict(wsb=gneed - 1), dict(ws=one + 4))
    for kw in grid:
        assert grid_count(**kw) == -1, kw
        assert grid_fill(**kw) == -1, kw
        assert query(**kw) == -1, kw
    assert L.slack((1000.0, 0.0, 0.0), 0.0625, (4, 4, 4))[1] > 0.0610                  # ... which is where 0.05 and 0.06 fall short
    assert L.slack((1000.0, 0.0, 0.0), 0.0625, (4, 4, 4))[1] < 0.0625
    assert grid_count(tot=None) == -1 and grid_fill(ne=-1) == -1 and grid_fill(ent=None) == -1
    for kw in (dict(nv=2 ** 31), dict(nf=2 ** 31)):
        assert grid_count(**kw) == -5 and grid_fill(**kw) == -5 and query(**kw) == -5, kw
    assert grid_fill(ne=2 ** 31) == -5 and query(ne=2 ** 31) == -5 and query(np=2 ** 31) == -5
    for kw in (dict(p=None), dict(d2=None), dict(face=None), dict(ent=None), dict(np=-1), dict(ne=-1), dict(md=-1.0), dict(md=float("nan"))):
        assert query(**kw) == -1, kw

    sneed = lib.ngp_meshdist_stats_workspace_bytes(7)
    nine = L.floats([0.1] * 9)
    for kw in (dict(d2=None), dict(face=None), dict(wts=None), dict(ws=None), dict(out=None), dict(n=0), dict(n=-1), dict(nt=9, th=nine),
               dict(nt=-1), dict(nt=2, th=None), dict(th=L.floats((0.1, -0.5))), dict(th=L.floats((float("nan"), 0.5))), dict(wsb=sneed - 1),
               dict(ws=one + 4)):
        assert stats(**kw) == -1, kw
    assert stats(n=2 ** 31) == -5
    s, m = C.c_float(), C.c_float()
    assert lib.ngp_meshdist_slack(origin, 0.25, 4, 4, 4, None, C.byref(m)) == -1 and lib.ngp_meshdist_slack(None, 0.25, 4, 4, 4, C.byref(s), C.byref(m)) == -1
    assert lib.ngp_meshdist_slack(origin, 0.25, 4, 1025, 4, C.byref(s), C.byref(m)) == -1


def test_too_many_cells_is_refused_by_the_size_query_and_the_entry_points():
    from ngp_pl_amd import _meshdist_lib as L
    lib = L.lib()
    assert lib.ngp_meshdist_grid_workspace_bytes(1024, 1024, 1024) == 8 * (2 ** 30 // 2048) + 4 * (2 ** 30 + 1) + 4 * 2 ** 30
    # 1024 x 1024 x 1024 is the limit; no axis may pass 1024, so "too many cells" can only be met through an axis out of range
    assert lib.ngp_meshdist_grid_workspace_bytes(1025, 1024, 1024) == 0
    s, m = C.c_float(), C.c_float()
    assert lib.ngp_meshdist_slack(L.floats((0, 0, 0)), 1.0, 1025, 1024, 1024, C.byref(s), C.byref(m)) == -1


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    from ngp_pl_amd import mesh
    m = mesh.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="CUDA"):
        mesh.sample_surface(m, 0.5)
    with pytest.raises(RuntimeError, match="CUDA"):
        mesh.closest_on_mesh(torch.zeros(2, 3), m)
    with pytest.raises(RuntimeError, match="CUDA"):
        mesh.mesh_distance(m, m)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mesh.sample_surface(m, bad)
    with pytest.raises(ValueError):
        mesh.mesh_distance(m, m, thresholds=[0.1] * 9)
    with pytest.raises(ValueError):
        mesh.mesh_distance(m, m, thresholds=[-0.1])


def test_grid_plan_respects_the_limits():
    from ngp_pl_amd import _meshdist_lib as L, mesh
    for extent, cell in (([0, 0, 0, 1, 1, 1, 0.01], None), ([0, 0, 0, 1, 1, 1, 1e-5], None), ([-5, 2, 0, 5, 2, 0.1, 0.3], 1e-9),
                         ([100, 100, 100, 101, 101, 101, 1e-4], None), ([float("inf")] * 3 + [float("-inf")] * 3 + [float("nan")], None)):
        origin, c, dims = mesh._plan_grid(extent, cell)
        assert all(1 <= n <= L.MAX_AXIS for n in dims) and dims[0] * dims[1] * dims[2] <= L.MAX_CELLS
        assert c >= L.slack(origin, c, dims)[1]
        if math.isfinite(extent[0]):
            for k in range(3):                     # the padded box is inside the grid
                assert origin[k] < extent[k] and extent[3 + k] < origin[k] + dims[k] * c
    assert mesh._plan_grid([0, 0, 0, 1, 1, 1, 0.01], None)[1] == float(F(0.02))


# ---- 2. the restatement against known answers

A0, B0, C0 = np.array([[0, 0, 0]], F), np.array([[1, 0, 0]], F), np.array([[0, 1, 0]], F)


def test_a_point_over_each_of_the_seven_regions_of_the_unit_right_triangle():
    cases = (((-1, -1, 1), 0, math.sqrt(3.0), (0, 0, 0)), ((2, 0.5, 0), 1, math.sqrt(1.25), (1, 0, 0)), ((0.5, -1, 0), 2, 1.0, (0.5, 0, 0)),
             ((0, 2, 1), 3, math.sqrt(2.0), (0, 1, 0)), ((-1, 0.5, 0), 4, 1.0, (0, 0.5, 0)), ((1, 1, 0), 5, math.sqrt(0.5), (0.5, 0.5, 0)),
             ((0.25, 0.25, 2), 6, 2.0, (0.25, 0.25, 0)))
    for p, case, dist, q in cases:
        got_q, d2, got_case = R.closest_f32(np.array([p], F), A0, B0, C0)
        assert int(got_case[0, 0]) == case, p
        assert np.array_equal(got_q[0, 0], np.array(q, F)), p
        assert d2.dtype == F and float(d2[0, 0]) == float(F(dist * dist)), p            # every d2 here is a short binary fraction
        assert abs(R.distance_f64(p, A0[0], B0[0], C0[0]) - dist) < 1e-15, p
    # permuting the corners moves the cases and keeps the distances
    for p, _, dist, _ in cases:
        for a, b, c in ((B0, C0, A0), (C0, A0, B0), (A0, C0, B0)):
            assert float(R.closest_f32(np.array([p], F), a, b, c)[1][0, 0]) == float(F(dist * dist))


def test_degenerate_and_non_finite_faces_contribute_nothing_and_ties_go_to_the_smaller_index():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [1, 1, 0]], F)
    f = np.array([[0, 1, 3], [0, 1, 5], [-1, 1, 2], [1, 4, 2], [0, 1, 2], [0, 1, 2]], np.int32)
    assert R.usable(v, f).tolist() == [False, False, False, True, True, True]
    d2, face, q = R.query_f32(np.array([[0.25, 0.25, 1], [0.9, 0.9, 0.5], [0.5, 0.5, 3]], F), v, f)
    assert face.tolist() == [4, 3, 3] and d2.tolist() == [1.0, 0.25, 9.0]                # the diagonal is shared by faces 3, 4 and 5
    assert np.array_equal(q, np.array([[0.25, 0.25, 0], [0.9, 0.9, 0], [0.5, 0.5, 0]], F))
    d2, face, q = R.query_f32(np.array([[0.25, 0.25, 1]], F), v, f, max_dist=0.5)
    assert face.tolist() == [-1] and np.isinf(d2).all() and np.isnan(q).all()
    assert R.query_f32(np.array([[0.25, 0.25, 1]], F), v, f, max_dist=1.0)[1].tolist() == [4]
    assert R.query_f32(np.array([[0.25, 0.25, 1]], F), v, f[:3])[1].tolist() == [-1]
    assert R.query_f32(np.array([[np.nan, 0.25, 1]], F), v, f)[1].tolist() == [-1]


def _lattice_centroids(k):
    """3k times the barycentric coordinates of the centroids of the k * k sub-triangles, from the lattice of the subdivision."""
    pts = lambda i, j: (k - i, i - j, j)                     # row i from A, position j: weights of (A, B, C) times k
    out = set()
    for i in range(k):
        for j in range(i + 1):
            out.add(tuple(sum(x) for x in zip(pts(i, j), pts(i + 1, j), pts(i + 1, j + 1))))
            if j < i:
                out.add(tuple(sum(x) for x in zip(pts(i, j), pts(i, j + 1), pts(i + 1, j + 1))))
    return out


def test_sampler_centroids_match_literal_barycentrics():
    literal = {1: [(1, 1, 1)],
               2: [(4, 1, 1), (1, 4, 1), (2, 2, 2), (1, 1, 4)],
               3: [(7, 1, 1), (4, 4, 1), (5, 2, 2), (4, 1, 4), (1, 7, 1), (2, 5, 2), (1, 4, 4), (2, 2, 5), (1, 1, 7)]}
    v = np.array([[0, 0, 0], [6, 0, 0], [0, 6, 3]], F)
    f = np.array([[0, 1, 2]], np.int32)
    for k, spacing in ((1, 10.0), (2, 5.0), (3, 3.2)):       # the longest edge is sqrt(81) = 9
        assert [R.barycentric_integers(k, s) for s in range(k * k)] == literal[k]
        assert set(literal[k]) == _lattice_centroids(k) and len(literal[k]) == k * k
        pts, wts, ids, counts = R.sample_f32(v, f, spacing)
        assert counts.tolist() == [k * k] and ids.tolist() == [0] * (k * k)
        want = np.array([[6.0 * j / (3 * k), 6.0 * l / (3 * k), 3.0 * l / (3 * k)] for _, j, l in literal[k]])
        assert np.array_equal(pts, want.astype(F)) and np.abs(pts - want).max() < 1e-6
    for k in (4, 7, 64):
        got = {R.barycentric_integers(k, s) for s in range(k * k)}
        assert got == _lattice_centroids(k) and all(sum(t) == 3 * k for t in got)


def test_sampler_k_is_clamped_and_weights_sum_to_the_area():
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [np.inf, 0, 0]], F)
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4], [2, 1, 0]], np.int32)
    diag = float(np.sqrt(F(32)))
    for spacing, k in ((100.0, 1), (diag, 1), (diag * 0.999, 2), (diag / 4, 4), (diag / 64, 64), (1e-3, 64), (1e-30, 64)):
        pts, wts, ids, counts = R.sample_f32(v, f, spacing)
        assert counts.tolist() == [k * k, 0, 0, k * k], spacing
        assert ids.tolist() == [0] * (k * k) + [3] * (k * k)
        assert math.fsum(wts[:k * k].astype(np.float64)) == 8.0 and float(wts[0]) == 8.0 / (k * k)      # area 8: exact for k a power of two
    assert int(R.subdivision(A0, B0, C0, F(np.nan))[0]) == 1


# ---- 3. the f32 rule against the float64 definition, within the bound the header derives


def _pairs(n, seed):
    """n (p, a, b, c) pairs: generic triangles, needles (one corner within 1e-3 of the opposite edge), points at 1e-3 of the
    coordinate magnitude from the face, and all of them again moved to a coordinate magnitude of 10."""
    g = np.random.RandomState(seed)
    a, b, c, p = (g.uniform(-1, 1, (n, 3)) for _ in range(4))
    kind = np.arange(n) % 4
    needle = (kind == 1) | (kind == 3)
    t = g.uniform(0, 1, (n, 1))
    c = np.where(needle[:, None], a + t * (b - a) + 1e-3 * g.uniform(-1, 1, (n, 3)), c)
    close = kind >= 2
    w = g.dirichlet((1, 1, 1), n)
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    on = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c
    p = np.where(close[:, None], on + 1e-3 * nrm * g.choice([-1.0, 1.0], (n, 1)), p)
    shift = np.where((np.arange(n) // 4 % 2 == 1)[:, None], g.uniform(8, 9, (n, 3)), 0.0)
    return tuple((x + shift).astype(F) for x in (p, a, b, c))


def test_f32_rule_against_the_float64_definition_within_the_derived_bound():
    p, a, b, c = _pairs(10000, 5)
    worst_lo = worst_hi = 0.0
    for begin in range(0, len(p), 100):
        sl = slice(begin, begin + 100)
        _, d2, _ = R.closest_f32(p[sl], a[sl], b[sl], c[sl])
        got = np.sqrt(np.diagonal(d2).astype(np.float64))
        for k in range(100):
            i = begin + k
            want = R.distance_f64(p[i], a[i], b[i], c[i])
            m = max(np.abs(x[i]).max() for x in (p, a, b, c))
            lo, hi = R.lower_error(float(m)), R.upper_error(p[i], a[i], b[i], c[i])
            assert want - lo <= got[k] <= want + hi, (i, want, got[k], lo, hi)
            worst_lo, worst_hi = max(worst_lo, (want - got[k]) / lo), max(worst_hi, (got[k] - want) / hi)
    print("worst share of the lower bound used: %.3f, of the upper bound: %.3f" % (worst_lo, worst_hi))


def test_statistics_restatement_on_a_hand_case():
    d2 = np.array([0.25, 1.0, np.inf, 4.0], F)
    face = np.array([3, 0, -1, 7], np.int32)
    w = np.array([1.0, 2.0, 8.0, 0.5], F)
    out, _ = R.stats_fsum(d2, face, w, (0.5, 1.0))
    assert out == [3.5, 0.5 + 2.0 + 1.0, 0.25 + 2.0 + 2.0, 2.0, 8.0, 1.0, 1.0, 3.0, 0, 0, 0, 0, 0, 0]


# ---- 4. the PLY reader


def test_load_ply_reads_what_save_ply_writes_bit_for_bit(tmp_path):
    from ngp_pl_amd import mesh
    g = np.random.RandomState(2)
    v = torch.from_numpy(g.randn(7, 3).astype(F))
    f = torch.from_numpy(g.randint(0, 7, (5, 3)).astype(np.int32))
    n = torch.from_numpy(g.randn(7, 3).astype(F))
    c = torch.from_numpy((g.randint(0, 256, (7, 3)) / 255.0).astype(F))
    for k, m in enumerate((mesh.Mesh(v, f), mesh.Mesh(v, f, n), mesh.Mesh(v, f, None, c), mesh.Mesh(v, f, n, c), mesh.Mesh(v[:0], f[:0]))):
        first, second = str(tmp_path / ("a%d.ply" % k)), str(tmp_path / ("b%d.ply" % k))
        mesh.save_ply(first, m)
        back = mesh.load_ply(first)
        assert torch.equal(back.vertices.view(torch.int32), m.vertices.view(torch.int32)) and torch.equal(back.faces, m.faces)
        assert (back.normals is None) == (m.normals is None) and (back.colors is None) == (m.colors is None)
        if m.normals is not None:
            assert torch.equal(back.normals.view(torch.int32), m.normals.view(torch.int32))
        if m.colors is not None:
            assert torch.equal(back.colors, m.colors)
        mesh.save_ply(second, back)
        assert open(first, "rb").read() == open(second, "rb").read()


def test_load_ply_refuses_anything_else(tmp_path):
    from ngp_pl_amd import mesh
    good = str(tmp_path / "good.ply")
    mesh.save_ply(good, mesh.Mesh(torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)))
    blob = open(good, "rb").read()
    quad = blob[:-13] + b"\x04" + blob[-12:]
    variants = {"ascii": blob.replace(b"binary_little_endian", b"ascii"), "big": blob.replace(b"binary_little_endian", b"binary_big_endian"),
                "double": blob.replace(b"property float x", b"property double x"), "short": blob[:-1], "long": blob + b"\x00",
                "extra": blob.replace(b"element face", b"property float quality\nelement face"), "quad": quad,
                "noply": b"solid\n" + blob, "uint": blob.replace(b"list uchar int", b"list uchar uint"),
                "edges": blob.replace(b"end_header", b"element edge 0\nend_header")}
    for name, data in variants.items():
        path = str(tmp_path / (name + ".ply"))
        with open(path, "wb") as out:
            out.write(data)
        with pytest.raises(ValueError, match=re.escape(path)):
            mesh.load_ply(path)
