"""CPU: the numpy restatement of the brick-sparse marching cubes (tests/mesh_sparse_reference.py) against the dense restatement and
against a brute-force statement of the occupancy rule, and the C ABI of libngp_meshsparse.so (header, exports, ctypes, code object,
build entry, the workspace formulas, host-side refusals of every entry point), the Python API's and the CLI's argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mc_reference as R
from tests import mesh_sparse_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN = os.path.join(ROOT, "ngp_pl_amd", "csrc", "meshsparse")           # the header lies beside the sources
HEADER = os.path.join(OWN, "ngp_meshsparse.h")
ENTRY_POINTS = ("abi_version", "build_arch", "mask", "index_workspace_bytes", "index_count", "index_fill", "points", "workspace_bytes",
                "count", "emit")
KERNELS = (b"sp_mask_small", b"sp_mask_box", b"sp_dilate", b"sp_scan_packed", b"sp_index_fill", b"sp_points", b"sp_count",
           b"sp_emit_vertices", b"sp_emit_faces")


def align256(x):
    return (x + 255) & ~255


# ---- 1. the restatement


def noise(shape, seed):
    return np.random.RandomState(seed).rand(*shape).astype(np.float32)


@pytest.mark.parametrize("shape", [(22, 13, 17), (9, 9, 9), (8, 16, 10)])
def test_all_true_mask_is_the_dense_restatement(shape):
    vol = noise(shape, 1)
    lo, hi = (-0.3, -0.5, 0.1), (0.7, 0.25, 1.3)
    v, f, n, _ = R.marching_cubes(vol, 0.5, lo, hi)
    sv, sf, sn, keys, cell = SR.restrict(vol, 0.5, lo, hi, np.ones(SR.brick_dims(shape), bool))
    assert len(f) > 100
    assert np.array_equal(sv, v) and np.array_equal(sf, f) and np.array_equal(sn, n, equal_nan=True)
    assert (np.diff(keys) > 0).all() and (np.diff(cell) >= 0).all()
    # a key names the vertex's owner and axis: the position lies on that edge
    nz, ny, nx = shape
    p, axis = keys // 3, keys % 3
    idx = np.stack([p % nx, (p // nx) % ny, p // (nx * ny)], 1)
    h = R.spacing(shape, lo, hi)
    a = np.asarray(lo, np.float32) + idx.astype(np.float32) * h
    other = np.arange(3)[None] != axis[:, None]
    assert np.array_equal(sv[other], a[other])


def test_restriction_keeps_the_faces_of_the_meshed_bricks_and_their_vertices():
    shape = (25, 20, 33)
    vol = noise(shape, 2)
    mask = np.random.RandomState(3).rand(*SR.brick_dims(shape)) < 0.5
    v, f, n, _ = R.marching_cubes(vol, 0.5, (0, 0, 0), (1, 1, 1))
    sv, sf, sn, keys, cell = SR.restrict(vol, 0.5, (0, 0, 0), (1, 1, 1), mask)
    nz, ny, nx = shape
    cx, cy, cz = cell % nx, (cell // nx) % ny, cell // (nx * ny)
    assert mask[cz // 8, cy // 8, cx // 8].all() and 0 < len(sf) < len(f)
    assert len(np.unique(sf)) == len(sv) and sf.max() == len(sv) - 1
    # the same triangles in space as the dense faces of those cells
    fz, fy, fx = SR.face_cells(vol, 0.5)
    keep = mask[fz // 8, fy // 8, fx // 8]
    assert np.array_equal(sv[sf], v[f[keep]])
    assert SR.restrict(vol, 0.5, (0, 0, 0), (1, 1, 1), np.zeros_like(mask))[1].shape == (0, 3)


def test_dilation_by_hand():
    m = np.zeros((3, 4, 5), bool)
    m[0, 0, 0] = m[2, 3, 4] = True
    d = SR.dilate(m)
    want = np.zeros_like(m)
    want[:2, :2, :2] = True
    want[1:, 2:, 3:] = True
    assert np.array_equal(d, want)
    assert np.array_equal(SR.dilate(np.ones((2, 2, 2), bool)), np.ones((2, 2, 2), bool)) and not SR.dilate(np.zeros((2, 3, 2), bool)).any()


def brute_force_mask(set_cells, cascades, G, scale, shape, lo, hi, margin):
    """Does the box of any set cell of the brick's cascade meet the grown box?  Cells are half-open [a, b) and the border cells
    reach to infinity (the clamp).  Written with plain Python floats: the test's numbers are dyadic, so everything is exact."""
    nz, ny, nx = shape
    n = (nx, ny, nz)
    nb = [(m + 7) // 8 for m in n]
    h = [(float(hi[a]) - float(lo[a])) / (n[a] - 1) for a in range(3)]
    out = np.zeros((nb[2], nb[1], nb[0]), bool)
    for bz in range(nb[2]):
        for by in range(nb[1]):
            for bx in range(nb[0]):
                b = (bx, by, bz)
                g0 = [lo[a] + 8 * b[a] * h[a] - margin * h[a] for a in range(3)]
                g1 = [lo[a] + min(8 * b[a] + 8, n[a] - 1) * h[a] + margin * h[a] for a in range(3)]
                bounds = [min(2.0 ** (k - 1), scale) for k in range(cascades)]
                inside = [k for k in range(cascades) if all(-bounds[k] <= g0[a] and g1[a] <= bounds[k] for a in range(3))]
                k = inside[0] if inside else cascades - 1
                s = bounds[k]
                w = 2 * s / G
                for kk, cx, cy, cz in set_cells:
                    if kk != k:
                        continue
                    meets = True
                    for a, c in enumerate((cx, cy, cz)):
                        left = -np.inf if c == 0 else -s + c * w
                        right = np.inf if c == G - 1 else -s + (c + 1) * w
                        meets = meets and g0[a] < right and left <= g1[a]
                    out[bz, by, bx] |= meets
    return out


@pytest.mark.parametrize("margin", [0, 1, 3])
@pytest.mark.parametrize("scale,cascades", [(0.5, 1), (2.0, 3)])
def test_occupancy_rule_against_brute_force(scale, cascades, margin):
    G = 8
    g = np.random.RandomState(7 + cascades)
    meshed = 0
    for shape, lo, hi in (((17, 17, 17), (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)),            # h = 1/16, the whole cascade-0 box
                          ((33, 9, 17), (-0.25, 0.0, -0.5), (0.25, 0.25, 0.0)),           # h = 1/64, 1/32, 1/32
                          ((33, 33, 17), (-scale, -scale, -scale), (scale, scale, scale)),  # the model's box: straddles cascades
                          ((65, 17, 9), (-0.375, -0.25, 0.125), (0.125, 0.25, 0.375))):
        if max(abs(x) for x in lo + hi) > scale:
            continue
        cells = [(int(g.randint(cascades)),) + tuple(int(c) for c in g.randint(0, G, 3)) for _ in range(6)]
        cells += [(k, c, c, c) for k in range(cascades) for c in (0, G - 1)]
        bits = SR.set_bits(cascades, G, cells)
        got = SR.occupancy_mask(bits, cascades, G, scale, shape, lo, hi, margin)
        want = brute_force_mask(cells, cascades, G, scale, shape, lo, hi, margin)
        assert got.shape == SR.brick_dims(shape) and np.array_equal(got, want), (shape, margin)
        assert not SR.occupancy_mask(np.zeros_like(bits), cascades, G, scale, shape, lo, hi, margin).any()
        meshed += int(got.sum()) * (not got.all())
    assert meshed > 0


def test_bit_order_is_the_marchers():
    # cell (cx, cy, cz) = (1, 0, 0) is morton 1, (0, 1, 0) is 2, (0, 0, 1) is 4: bits 1, 2, 4 of byte 0; cascade 1 starts at byte G^3 / 8
    G = 4
    assert SR.set_bits(2, G, [(0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)])[0] == 0b10110
    bits = SR.set_bits(2, G, [(1, 3, 2, 1)])
    grids = SR.occupancy_grids(bits, 2, G)
    assert grids.sum() == 1 and grids[1, 1, 2, 3] and np.nonzero(bits)[0].tolist() == [G ** 3 // 8 + int(SR.morton(3, 2, 1)) // 8]


# ---- 2. the C ABI


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (\w+)", out))


def test_header_compiles_as_c99_alone_and_beside_the_others():
    include = os.path.join(ROOT, "include")
    others = tuple(sorted(n for n in os.listdir(include) if n.endswith(".h")))
    for src in ('#include "ngp_meshsparse.h"\nint main(void) { return 0; }\n',
                "".join('#include "%s"\n' % n for n in others + ("ngp_meshsparse.h",)) + "int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n",
                "".join('#include "%s"\n' % n for n in ("ngp_meshsparse.h",) + others[::-1]) + "int main(void) { return NGP_MESHSPARSE_BRICK; }\n"):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", include, "-I", OWN, "-x", "c", "-"],
                           input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == {"stddef.h", "stdint.h"}
    assert "#ifndef NGP_EINVAL" in text and "#ifndef NGP_ERANGE" in text and "THE CONTRACT" in text
    from ngp_pl_amd import _meshsparse_lib
    assert "#define NGP_MESHSPARSE_BRICK %d " % _meshsparse_lib.BRICK in text
    assert "#define NGP_MESHSPARSE_BRICK_POINTS %d" % _meshsparse_lib.BRICK_POINTS in text and _meshsparse_lib.BRICK ** 3 == _meshsparse_lib.BRICK_POINTS
    assert SR.BRICK == _meshsparse_lib.BRICK


def test_library_exports_exactly_its_header_and_no_symbol_of_another_library():
    from ngp_pl_amd import _abi, _mesh_lib, _meshsparse_lib
    protos = _abi.parse(HEADER)
    assert set(protos) == {"ngp_meshsparse_" + n for n in ENTRY_POINTS}
    own = _exports(_meshsparse_lib.LIB_PATH)
    assert own == set(protos) == set(_meshsparse_lib.exported_symbols())
    lib = _meshsparse_lib.lib()
    assert lib.ngp_meshsparse_abi_version() == 1 == _meshsparse_lib.ABI_VERSION and lib.ngp_meshsparse_build_arch() == b"gfx950"
    csrc = os.path.dirname(_meshsparse_lib.LIB_PATH)
    others = [os.path.join(csrc, n) for n in os.listdir(csrc) if n.startswith("libngp_") and n.endswith(".so") and n != "libngp_meshsparse.so"]
    assert len(others) >= 16
    for path in others:
        theirs = _exports(path)
        assert theirs and not theirs & own and not [s for s in theirs if s.startswith("ngp_meshsparse")], path
    # the dense extractor's library keeps its six entry points
    assert _exports(_mesh_lib.LIB_PATH) == set(_abi.parse(os.path.join(ROOT, "include", "ngp_mesh.h")))


def test_ctypes_agrees_with_the_header():
    from ngp_pl_amd import _abi, _meshsparse_lib
    protos = _abi.parse(HEADER)
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in _meshsparse_lib._PROTOS.items()) if m]
    assert not problems, "\n".join(problems)
    lib = _meshsparse_lib.lib()
    for name, pr in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and _abi.ctypes_agrees(list(f.argtypes), pr) is None, name
        want = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[pr.ret]
        assert f.restype is want, name


def test_code_object_is_gfx950_only_and_the_build_has_contraction_off():
    from ngp_pl_amd import _meshsparse_lib, build
    blob = open(_meshsparse_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob
    for kernel in KERNELS:
        assert kernel in blob, kernel
    assert build.MESHSPARSE_LIB == _meshsparse_lib.LIB_PATH and build.MESHSPARSE_CFLAGS == ["-ffp-contract=off"]
    assert build.MESHSPARSE_SOURCES == [os.path.join("meshsparse", "meshsparse.hip")]
    for rel in build.MESHSPARSE_SOURCES + build.MESHSPARSE_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, rel)), rel
    source = open(os.path.join(build.CSRC, build.MESHSPARSE_SOURCES[0])).read()
    includes = {"ngp_meshsparse.h", "../mesh/mc_tables.h", "../mesh_host.h", "../mesh_scan.h", "../mesh_mc.h"}
    assert set(re.findall(r'#include\s*"([^"]+)"', source)) == includes
    assert set(os.path.basename(h) for h in build.MESHSPARSE_HEADERS) == {os.path.basename(i) for i in includes}
    # the dense extractor includes the same rules, and names them among its headers
    dense = open(os.path.join(build.CSRC, build.MESH_SOURCES[0])).read()
    assert '#include "../mesh_mc.h"' in dense and "mesh_mc.h" in build.MESH_HEADERS


def test_workspace_formulas_and_argument_validation_need_no_gpu():
    from ngp_pl_amd import _lib, _meshsparse_lib
    lib = _meshsparse_lib.lib()
    # 5 B per sampled point and 20 B per sampled brick, each array rounded up to 256 B
    for m, s in ((0, 1), (1, 1), (3, 10), (1000, 4097), (2 ** 30, 2 ** 30)):
        want = align256(512 * s) + align256(2048 * s) + align256(4 * s) + 2 * align256(8 * s)
        assert lib.ngp_meshsparse_workspace_bytes(m, s) == want
        assert 2580 * s <= want < 2580 * s + 5 * 256
    for m, s in ((0, 0), (-1, 5), (6, 5), (1, 2 ** 30 + 1), (1, -1)):
        assert lib.ngp_meshsparse_workspace_bytes(m, s) == 0
    for n in ((64, 64, 64), (22, 13, 17), (2, 2, 2), (65535, 9, 9), (4097, 4097, 4097), (8192, 8192, 8192)):
        B = int(np.prod([(k + 7) // 8 for k in n]))
        K = (B + 2047) // 2048
        assert lib.ngp_meshsparse_index_workspace_bytes(*n) == align256(B) + align256(4 * K) + 2 * align256(8 * K), n
    for n in ((1, 64, 64), (64, 65536, 64), (64, 64, 0), (8200, 8192, 8192), (65535, 65535, 65535)):        # an axis, or more than 2^30 bricks
        assert lib.ngp_meshsparse_index_workspace_bytes(*n) == 0, n
    fake = C.c_void_p(4096)          # never dereferenced: every call below is rejected before a launch
    b6 = (C.c_float * 6)(0, 0, 0, 1, 1, 1)
    flat = (C.c_float * 6)(0, 0, 0, 1, 0, 1)
    nan6 = (C.c_float * 6)(0, 0, 0, 1, float("nan"), 1)
    N = (64, 64, 64)
    iws = lib.ngp_meshsparse_index_workspace_bytes(*N)
    M, S = 10, 40
    ws = lib.ngp_meshsparse_workspace_bytes(M, S)
    nan, inf = float("nan"), float("inf")

    def mask(bits=fake, cascades=1, G=128, scale=0.5, n=N, b=b6, margin=1.0, out=fake):
        return ("ngp_meshsparse_mask", bits, cascades, G, scale) + n + (b, margin, out, None)

    def icount(m=fake, n=N, w=fake, wb=iws, counts=fake):
        return ("ngp_meshsparse_index_count", m) + n + (w, wb, counts, None)

    def ifill(m=fake, n=N, w=fake, wb=iws, nm=M, ns=S, table=fake, mb=fake, sb=fake):
        return ("ngp_meshsparse_index_fill", m) + n + (w, wb, nm, ns, table, mb, sb, None)

    def points(n=N, b=b6, sb=fake, ns=S, begin=0, count=S, xyz=fake):
        return ("ngp_meshsparse_points",) + n + (b, sb, ns, begin, count, xyz, None)

    def count(pool=fake, n=N, mm=fake, table=fake, mb=fake, nm=M, sb=fake, ns=S, w=fake, wb=ws, totals=fake):
        return ("ngp_meshsparse_count", pool) + n + (20.0, mm, table, mb, nm, sb, ns, w, wb, totals, None)

    def emit(pool=fake, n=N, b=b6, table=fake, mb=fake, nm=M, sb=fake, ns=S, w=fake, wb=ws, nv=5, nf=5, v=fake, nrm=fake, key=fake, f=fake,
             cell=fake):
        return ("ngp_meshsparse_emit", pool) + n + (20.0, b, table, mb, nm, sb, ns, w, wb, nv, nf, v, nrm, key, f, cell, None)

    bad = [
        mask(bits=None), mask(b=None), mask(out=None), mask(cascades=0), mask(cascades=33), mask(G=1), mask(G=96), mask(G=2048), mask(scale=0.0),
        mask(scale=-1.0), mask(scale=nan), mask(scale=inf), mask(margin=-1.0), mask(margin=nan), mask(margin=inf), mask(b=flat), mask(b=nan6),
        mask(n=(1, 64, 64)), mask(n=(64, 64, 65536)), mask(n=(8200, 8192, 8192)),
        icount(m=None), icount(w=None), icount(counts=None), icount(wb=iws - 1), icount(n=(64, 1, 64)), icount(n=(70000, 64, 64)),
        ifill(m=None), ifill(w=None), ifill(table=None), ifill(mb=None), ifill(sb=None), ifill(wb=iws - 1), ifill(nm=-1), ifill(nm=S + 1),
        ifill(ns=8 ** 3 + 1), ifill(n=(64, 64, 1)),
        points(b=None), points(sb=None), points(xyz=None), points(ns=-1), points(ns=8 ** 3 + 1), points(begin=-1), points(count=-1),
        points(begin=1), points(count=S + 1), points(begin=S + 1, count=0), points(begin=2 ** 62, count=2 ** 62), points(b=flat), points(b=nan6),
        points(n=(1, 64, 64)),
        count(pool=None), count(mm=None), count(table=None), count(mb=None), count(sb=None), count(w=None), count(totals=None), count(wb=ws - 1),
        count(nm=-1), count(nm=S + 1), count(ns=0), count(ns=8 ** 3 + 1, wb=2 ** 40), count(n=(64, 64, 70000)),
        emit(pool=None), emit(b=None), emit(table=None), emit(mb=None), emit(sb=None), emit(w=None), emit(v=None), emit(f=None), emit(wb=ws - 1),
        emit(nv=-1), emit(nf=-1), emit(nm=S + 1), emit(ns=0), emit(b=flat), emit(b=nan6), emit(n=(1, 64, 64)),
    ]
    for args in bad:
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _meshsparse_lib.call(*args)
    for args in (emit(nv=2 ** 31), emit(nf=2 ** 31)):
        with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
            _meshsparse_lib.call(*args)
    # nothing to do: no launch
    assert _meshsparse_lib.call(*emit(nv=0, nf=0, v=None, nrm=None, key=None, f=None, cell=None)) == 0
    assert _meshsparse_lib.call(*points(count=0, xyz=None)) == 0 and _meshsparse_lib.call(*points(begin=S, count=0)) == 0


# ---- 3. the Python API's checks and the CLI


def test_python_api_argument_checks():
    import torch
    from ngp_pl_amd import mesh
    assert [fl.name for fl in mesh.dataclasses.fields(mesh.SparseVolume)] == ["resolution", "mask", "brick_table", "mesh_bricks", "sample_bricks",
                                                                             "pool"]
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.SparseVolume.from_dense(torch.zeros(9, 9, 9), torch.ones(2, 2, 2, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.SparseVolume.index(9, torch.ones(2, 2, 2, dtype=torch.bool))
    for bad in (torch.ones(2, 2, 3, dtype=torch.bool), torch.ones(2, 2, 2), np.ones((2, 2, 2), bool)):
        with pytest.raises(ValueError, match="mask"):
            mesh.SparseVolume.index(9, bad)
    with pytest.raises(ValueError, match="SparseVolume"):
        mesh.marching_cubes_sparse(torch.zeros(9, 9, 9))
    for sparse in (1, "yes", dict(margin=1), dict(margin_voxels=-1), dict(margin_voxels=float("nan")), dict(margin_voxels="1"), [True]):
        with pytest.raises(ValueError, match="sparse"):
            mesh.extract_mesh(None, 8, sparse=sparse)
    with pytest.raises(ValueError, match="sparse and tsdf"):
        mesh.extract_mesh(None, 8, sparse=True, tsdf=dict(K=None, poses=None, img_wh=(4, 4)))
    assert mesh._sparse_options(False) is None and mesh._sparse_options(None) is None
    assert mesh._sparse_options(True) == dict(mask=None, margin_voxels=1) == mesh._sparse_options({})


def test_cli_lists_the_options_and_refuses_bad_combinations(capsys):
    from ngp_pl_amd import mesh
    with pytest.raises(SystemExit) as e:
        mesh.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--sparse", "--sparse-margin-voxels M"):
        assert flag in out
    for bad in (["--sparse-margin-voxels", "2"], ["--sparse", "--sparse-margin-voxels", "-1"], ["--sparse", "--sparse-margin-voxels", "nan"],
                ["--sparse", "--tsdf-cameras", "cams.npz"]):
        with pytest.raises(SystemExit) as e:
            mesh.main(["--ckpt", "x", "--out", "y.ply"] + bad)
        assert e.value.code == 2, bad
        assert "--sparse" in capsys.readouterr().err
