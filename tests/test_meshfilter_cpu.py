"""CPU: the C ABI of libngp_meshfilter.so (header, exports, ctypes, code object, host-side argument checks), the numpy
restatement the GPU tests compare against (tests/mesh_components_reference.py), and the Python API's argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mc_reference as R
from tests import mesh_components_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngp_meshfilter.h")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (\w+)", out))


def test_header_compiles_as_c99_alone_and_after_the_other_two():
    for src in ('#include "ngp_meshfilter.h"\nint main(void) { return 0; }\n',
                '#include "ngp_hip.h"\n#include "ngp_mesh.h"\n#include "ngp_meshfilter.h"\nint main(void) { return NGP_EINVAL + NGP_ERANGE; }\n'):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            "-x", "c", "-"], input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == {"stddef.h", "stdint.h"}


def test_library_exports_exactly_its_header():
    from ngp_pl_amd import _abi, _meshfilter_lib
    protos = _abi.parse(HEADER)
    assert len(protos) == 6 and all(n.startswith("ngp_meshfilter_") for n in protos)
    assert _exports(_meshfilter_lib.LIB_PATH) == set(protos)
    assert set(_meshfilter_lib.exported_symbols()) == set(protos)
    lib = _meshfilter_lib.lib()
    assert lib.ngp_meshfilter_abi_version() == 1 == _meshfilter_lib.ABI_VERSION and lib.ngp_meshfilter_build_arch() == b"gfx950"


def test_the_three_libraries_share_no_symbol():
    from ngp_pl_amd import _abi, _lib, _mesh_lib, _meshfilter_lib
    _lib.lib()
    _mesh_lib.lib()
    _meshfilter_lib.lib()
    own, main, mesh = _exports(_meshfilter_lib.LIB_PATH), _exports(_lib.LIB_PATH), _exports(_mesh_lib.LIB_PATH)
    assert own and main and mesh
    assert not own & (main | mesh)
    assert not [s for s in main | mesh if s.startswith("ngp_meshfilter")]
    assert not [s for s in own if not s.startswith("ngp_meshfilter_")]
    declared_elsewhere = set(_abi.parse_all()) | set(_abi.parse(os.path.join(ROOT, "include", "ngp_mesh.h")))
    assert not set(_abi.parse(HEADER)) & declared_elsewhere


def test_ctypes_agrees_with_the_header():
    from ngp_pl_amd import _abi, _meshfilter_lib
    protos = _abi.parse(HEADER)
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in _meshfilter_lib._PROTOS.items()) if m]
    assert not problems, "\n".join(problems)
    lib = _meshfilter_lib.lib()
    for name, pr in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and _abi.ctypes_agrees(list(f.argtypes), pr) is None, name
        want = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[pr.ret]
        assert f.restype is want, name


def test_code_object_is_gfx950_only():
    from ngp_pl_amd import _meshfilter_lib
    blob = open(_meshfilter_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob


def test_argument_validation_needs_no_gpu():
    from ngp_pl_amd import _lib, _meshfilter_lib
    lib = _meshfilter_lib.lib()
    V, F = 100000, 180000
    ws = lib.ngp_meshfilter_workspace_bytes(V, F)
    assert 5 * V <= ws < 5 * V + 12 * ((V + F) // 2048 + 2) + 8 * 256          # 5 B per vertex, 12 B per block, alignment
    assert lib.ngp_meshfilter_workspace_bytes(0, 0) > 0
    assert lib.ngp_meshfilter_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1) > 5 * (2 ** 31 - 1)
    for v, f in ((-1, 5), (5, -1), (2 ** 31, 5), (5, 2 ** 31)):
        assert lib.ngp_meshfilter_workspace_bytes(v, f) == 0
    fake = C.c_void_p(4096)          # never dereferenced: every call below is rejected before a launch
    big = 2 ** 31
    bad = [
        ("ngp_meshfilter_label", None, V, F, fake, fake, fake, fake, None),                    # null faces
        ("ngp_meshfilter_label", fake, V, F, None, fake, fake, fake, None),                    # null vertex_label
        ("ngp_meshfilter_label", fake, V, F, fake, None, fake, fake, None),                    # null face_label
        ("ngp_meshfilter_label", fake, V, F, fake, fake, None, fake, None),                    # null component_faces
        ("ngp_meshfilter_label", fake, V, F, fake, fake, fake, None, None),                    # null n_components
        ("ngp_meshfilter_label", fake, -1, F, fake, fake, fake, fake, None),                   # negative counts
        ("ngp_meshfilter_label", fake, V, -1, fake, fake, fake, fake, None),
        ("ngp_meshfilter_count", None, fake, fake, V, F, fake, ws, fake, None),                # null faces
        ("ngp_meshfilter_count", fake, None, fake, V, F, fake, ws, fake, None),                # null vertex_label
        ("ngp_meshfilter_count", fake, fake, None, V, F, fake, ws, fake, None),                # null keep
        ("ngp_meshfilter_count", fake, fake, fake, V, F, None, ws, fake, None),                # null workspace
        ("ngp_meshfilter_count", fake, fake, fake, V, F, fake, ws, None, None),                # null totals
        ("ngp_meshfilter_count", fake, fake, fake, V, F, fake, ws - 1, fake, None),            # workspace too small
        ("ngp_meshfilter_count", fake, fake, fake, -1, F, fake, ws, fake, None),
        ("ngp_meshfilter_emit", None, fake, fake, fake, fake, fake, V, F, fake, ws, 1, 1, fake, fake, fake, fake, None),     # null faces
        ("ngp_meshfilter_emit", fake, None, fake, fake, fake, fake, V, F, fake, ws, 1, 1, fake, fake, fake, fake, None),     # null labels
        ("ngp_meshfilter_emit", fake, fake, None, fake, fake, fake, V, F, fake, ws, 1, 1, fake, fake, fake, fake, None),     # null keep
        ("ngp_meshfilter_emit", fake, fake, fake, None, fake, fake, V, F, fake, ws, 1, 1, fake, fake, fake, fake, None),     # null vertices
        ("ngp_meshfilter_emit", fake, fake, fake, fake, fake, fake, V, F, None, ws, 1, 1, fake, fake, fake, fake, None),     # null workspace
        ("ngp_meshfilter_emit", fake, fake, fake, fake, fake, fake, V, F, fake, ws - 1, 1, 1, fake, fake, fake, fake, None),  # small workspace
        ("ngp_meshfilter_emit", fake, fake, fake, fake, fake, fake, V, F, fake, ws, 1, 1, None, fake, fake, fake, None),     # null vertices_out
        ("ngp_meshfilter_emit", fake, fake, fake, fake, fake, fake, V, F, fake, ws, 1, 1, fake, None, fake, fake, None),     # normals without output
        ("ngp_meshfilter_emit", fake, fake, fake, fake, fake, None, V, F, fake, ws, 1, 1, fake, fake, fake, fake, None),     # colors_out without colors
        ("ngp_meshfilter_emit", fake, fake, fake, fake, fake, fake, V, F, fake, ws, 1, 1, fake, fake, fake, None, None),     # null faces_out
        ("ngp_meshfilter_emit", fake, fake, fake, fake, fake, fake, V, F, fake, ws, -1, 1, fake, fake, fake, fake, None),    # negative output size
        ("ngp_meshfilter_emit", fake, fake, fake, fake, fake, fake, V, F, fake, ws, V + 1, 1, fake, fake, fake, fake, None),  # more than the input
        ("ngp_meshfilter_emit", fake, fake, fake, fake, fake, fake, V, F, fake, ws, 1, F + 1, fake, fake, fake, fake, None),
    ]
    for args in bad:
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _meshfilter_lib.call(*args)
    too_big = [
        ("ngp_meshfilter_label", fake, big, F, fake, fake, fake, fake, None),
        ("ngp_meshfilter_label", fake, V, big, fake, fake, fake, fake, None),
        ("ngp_meshfilter_count", fake, fake, fake, big, F, fake, ws, fake, None),
        ("ngp_meshfilter_count", fake, fake, fake, V, big, fake, ws, fake, None),
        ("ngp_meshfilter_emit", fake, fake, fake, fake, fake, fake, big, F, fake, ws, 1, 1, fake, fake, fake, fake, None),
        ("ngp_meshfilter_emit", fake, fake, fake, fake, fake, fake, V, big, fake, ws, 1, 1, fake, fake, fake, fake, None),
    ]
    for args in too_big:
        with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
            _meshfilter_lib.call(*args)
    # zero-sized meshes and an empty result: nothing to launch
    assert _meshfilter_lib.call("ngp_meshfilter_label", None, 0, 0, None, None, None, None, None) == 0
    assert _meshfilter_lib.call("ngp_meshfilter_count", None, None, None, 0, 0, None, 0, None, None) == 0
    assert _meshfilter_lib.call("ngp_meshfilter_emit", None, None, None, None, None, None, 0, 0, None, 0, 0, 0, None, None, None, None, None) == 0
    assert _meshfilter_lib.call("ngp_meshfilter_emit", fake, fake, fake, fake, None, None, V, F, fake, ws, 0, 0, None, None, None, None, None) == 0


def test_python_api_rejects_cpu_tensors_and_bad_faces():
    import torch
    from ngp_pl_amd import mesh
    v = torch.zeros(4, 3)
    f = torch.zeros(2, 3, dtype=torch.int32)
    for fn in (lambda m: mesh.filter_components(m, keep_largest=1), lambda m: mesh.filter_components(m), mesh.connected_components):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(mesh.Mesh(v, f))
        for bad in (f.long(), f.float(), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(6, dtype=torch.int32), f.numpy()):
            with pytest.raises(ValueError):
                fn(mesh.Mesh(v, bad))
        with pytest.raises(ValueError):
            fn(mesh.Mesh(v.double(), f))
        with pytest.raises(ValueError):
            fn(mesh.Mesh(v, f, torch.zeros(5, 3)))


def blob_volume(n=48):
    """Five separated balls of different radii (smooth, so each iso-surface is one closed sphere-like sheet)."""
    balls = [((0.25, 0.25, 0.25), 0.17), ((0.75, 0.3, 0.3), 0.13), ((0.3, 0.75, 0.7), 0.15), ((0.75, 0.75, 0.75), 0.10), ((0.72, 0.3, 0.8), 0.06)]
    z, y, x = np.meshgrid(*[np.linspace(0, 1, n)] * 3, indexing="ij")
    v = np.zeros((n, n, n))
    for c, r in balls:
        v = np.maximum(v, r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2))
    return v.astype(np.float32), len(balls)


def test_reference_counts_the_blobs_and_keeps_a_closed_sphere():
    vol, n_blobs = blob_volume()
    v, f, nrm, _ = R.marching_cubes(vol, 0.0, (0, 0, 0), (1, 1, 1))
    c = CR.Components(f, len(v))
    assert c.n_components == n_blobs and c.faces_per_component.sum() == len(f)
    assert (c.vertex_label[c.labels] == c.labels).all()                     # a label is a member of its component
    assert (c.vertex_label <= np.arange(len(v))).all()                      # and its smallest index
    for i in range(3):
        assert np.array_equal(c.vertex_label[f[:, i]], c.face_label)
    assert (np.diff(c.faces_per_component[np.lexsort((c.labels, -c.faces_per_component))]) <= 0).all()
    ids = np.repeat(np.arange(len(v), dtype=np.float32)[:, None], 3, 1)        # rides along as "colours": where a vertex came from
    v1, f1, n1, id1 = CR.filter_components(v, f, nrm, ids, keep_largest=1)
    assert len(f1) == c.faces_per_component.max() and f1.max() + 1 == len(v1) == len(n1)
    assert R.is_closed_oriented(f1) and R.euler(v1, f1) == 2
    assert CR.Components(f1, len(v1)).n_components == 1
    # the largest ball is the one around (0.25, 0.25, 0.25), radius 0.17
    assert np.abs(np.linalg.norm(v1 - np.float32(0.25), axis=1) - 0.17).max() < 0.03
    # order-preserving: the kept vertices are a subsequence of the input's
    idx = id1[:, 0].astype(np.int64)
    assert (np.diff(idx) > 0).all() and np.array_equal(v[idx], v1) and np.array_equal(nrm[idx], n1)
    assert np.array_equal(idx[f1], f[c.face_label == c.labels[np.argmax(c.faces_per_component)]])      # faces in order, re-indexed
    for k in range(n_blobs + 2):
        assert CR.Components(CR.filter_components(v, f, keep_largest=k)[1], len(v)).n_components == min(k, n_blobs)
    va, fa, _, _ = CR.filter_components(v, f, keep_largest=n_blobs)
    assert np.array_equal(va, v) and np.array_equal(fa, f)


def test_reference_tie_break_and_min_faces_edges():
    # components by label: 0 (2 faces), 3 (1 face), 6 (2 faces), vertex 9 isolated, 10 (1 face, numbered downwards)
    f = np.array([[0, 1, 2], [2, 1, 0], [5, 4, 3], [6, 7, 8], [8, 7, 6], [12, 11, 10]], np.int32)
    v = np.arange(13 * 3, dtype=np.float32).reshape(13, 3)
    c = CR.Components(f, 13)
    assert c.labels.tolist() == [0, 3, 6, 10] and c.faces_per_component.tolist() == [2, 1, 2, 1] and c.n_components == 4
    assert c.vertex_label.tolist() == [0, 0, 0, 3, 3, 3, 6, 6, 6, 9, 10, 10, 10]
    assert c.face_label.tolist() == [0, 0, 3, 6, 6, 10]
    assert c.component_faces.tolist() == [2, 0, 0, 1, 0, 0, 2, 0, 0, 0, 1, 0, 0]
    assert CR.select(c, keep_largest=1).tolist() == [True, False, False, False]            # 0 and 6 tie: the smaller label
    assert CR.select(c, keep_largest=2).tolist() == [True, False, True, False]
    assert CR.select(c, keep_largest=3).tolist() == [True, True, True, False]              # 3 and 10 tie
    assert CR.select(c, keep_largest=0).tolist() == [False] * 4
    assert CR.select(c, min_faces=2).tolist() == [True, False, True, False]
    assert CR.select(c, min_faces=1).tolist() == [True] * 4 and CR.select(c, min_faces=0).tolist() == [True] * 4
    assert CR.select(c, min_faces=3).tolist() == [False] * 4
    assert CR.select(c, keep_largest=3, min_faces=2).tolist() == [True, False, True, False]
    assert CR.select(c, keep_largest=1, min_faces=3).tolist() == [False] * 4
    v2, f2, _, _ = CR.filter_components(v, f, keep_largest=3)
    assert np.array_equal(v2, v[:9]) and np.array_equal(f2, f[:5])                         # the isolated vertex goes too
    v3, f3, _, _ = CR.filter_components(v, f, min_faces=2)
    assert np.array_equal(v3, v[[0, 1, 2, 6, 7, 8]]) and f3.tolist() == [[0, 1, 2], [2, 1, 0], [3, 4, 5], [5, 4, 3]]
    v0, f0, _, _ = CR.filter_components(v, f, keep_largest=0)
    assert v0.shape == (0, 3) and f0.shape == (0, 3)
