"""Generator of the marching-cubes case tables (ngp_pl_amd/csrc/mesh/mc_tables.h), derived from cube topology.

Conventions (shared by the kernels and by tests/mc_reference.py):
  corner c = (x, y, z) = (c & 1, (c >> 1) & 1, (c >> 2) & 1); case index = sum of 1 << c over the corners that are inside.
  edge e joins corners EDGES[e] = (a, b), a < b, differing in one axis bit; axis = e // 4 (x, y, z).  Its vertex is owned by
  lattice corner a (a lattice point owns its +x, +y and +z edges).
Face rule: on each of the 6 faces the crossed edges pair up into segments.  With two crossed edges they form one segment; with
four (the two inside corners sit on a diagonal) each inside corner is cut off on its own -- inside corners stay separated.  The
rule reads a face's 4 corners only, so the two cells that share a face choose the same segments and the mesh has no cracks.
Each segment is directed so that (segment) x (face's outward normal) points to the inside corner(s); chained, the segments form
closed loops whose right-hand normal points from inside to outside.  Each loop is fan-triangulated from an apex chosen so that
no fan diagonal joins two vertices on one cube face (a neighbouring cell could otherwise emit the same diagonal: 4 triangles on
one mesh edge).

`python -m ngp_pl_amd.mc_tables` rewrites the header; tests/test_mesh_cpu.py checks the committed one is byte-identical.
"""
import os
import sys

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mesh", "mc_tables.h")


def corner_xyz(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def _edges():
    out = []
    for axis in range(3):
        bit = 1 << axis
        for a in range(8):
            if not a & bit:
                out.append((a, a | bit))
    return out


EDGES = _edges()                        # 12 x (corner a, corner b); edges 4*axis .. 4*axis+3 run along `axis`
EDGE_INDEX = {e: i for i, e in enumerate(EDGES)}


def _faces():
    """6 faces: (axis, side, 4 corners in cyclic order, outward normal)."""
    out = []
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for side in (0, 1):
            base = side << axis
            cyc = [base, base | (1 << u), base | (1 << u) | (1 << v), base | (1 << v)]
            n = [0, 0, 0]
            n[axis] = 1 if side else -1
            out.append((axis, side, cyc, tuple(n)))
    return out


FACES = _faces()


def _edge_of(a, b):
    return EDGE_INDEX[(min(a, b), max(a, b))]


def _mid(e):
    a, b = EDGES[e]
    pa, pb = corner_xyz(a), corner_xyz(b)
    return tuple((pa[i] + pb[i]) / 2.0 for i in range(3))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def face_segments(case, face):
    """Directed segments (edge, edge) the face rule prescribes on one face for one case."""
    _, _, cyc, n = face
    inside = [bool(case >> c & 1) for c in cyc]
    crossed = [(i, _edge_of(cyc[i], cyc[(i + 1) % 4])) for i in range(4) if inside[i] != inside[(i + 1) % 4]]
    if not crossed:
        return []
    if len(crossed) == 2:
        pairs = [(crossed[0][1], crossed[1][1], [cyc[i] for i in range(4) if inside[i]])]
    else:
        assert len(crossed) == 4
        pairs = []
        for i in range(4):
            if inside[i]:      # cut off this inside corner on its own: its two face edges
                pairs.append((_edge_of(cyc[i], cyc[(i + 1) % 4]), _edge_of(cyc[i], cyc[(i - 1) % 4]), [cyc[i]]))
    segs = []
    for e0, e1, ins in pairs:
        m0, m1 = _mid(e0), _mid(e1)
        s = tuple(m1[i] - m0[i] for i in range(3))
        mid = tuple((m0[i] + m1[i]) / 2 for i in range(3))
        pin = [corner_xyz(c) for c in ins]
        towards = tuple(sum(p[i] for p in pin) / len(pin) - mid[i] for i in range(3))
        side = _dot(_cross(s, n), towards)
        assert side != 0
        segs.append((e0, e1) if side > 0 else (e1, e0))
    return segs


def case_segments(case):
    return [s for f in FACES for s in face_segments(case, f)]


def sign_change_edges(case):
    return [e for e, (a, b) in enumerate(EDGES) if (case >> a & 1) != (case >> b & 1)]


def _faces_of_edge(e):
    a, b = EDGES[e]
    return {fi for fi, f in enumerate(FACES) if a in f[2] and b in f[2]}


def _share_face(e0, e1):
    return bool(_faces_of_edge(e0) & _faces_of_edge(e1))


def case_loops(case):
    segs = case_segments(case)
    nxt = {}
    for a, b in segs:
        assert a not in nxt, (case, "two segments leave edge %d" % a)
        nxt[a] = b
    assert sorted(nxt) == sorted(set(nxt.values())) == sign_change_edges(case), case
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        loops.append(loop)
    return loops


def fan(loop):
    """Triangles (v0, vi, vi+1) of the loop rotated to the first apex whose diagonals never join two edges of one face."""
    m = len(loop)
    for r in range(m):
        lp = loop[r:] + loop[:r]
        if all(not _share_face(lp[0], lp[i]) for i in range(2, m - 1)):
            return [(lp[0], lp[i], lp[i + 1]) for i in range(1, m - 1)]
    raise AssertionError("no admissible fan apex for loop %r" % loop)


def case_triangles(case):
    return [t for lp in case_loops(case) for t in fan(lp)]


def tables():
    tris = [case_triangles(c) for c in range(256)]
    edge_mask = [sum(1 << e for e in sign_change_edges(c)) for c in range(256)]
    max_tris = max(len(t) for t in tris)
    assert max_tris <= 8, max_tris
    # every crossed edge carries a vertex used by a triangle, and nothing else does
    for c in range(256):
        used = sorted({e for t in tris[c] for e in t})
        assert used == sign_change_edges(c), c
    return edge_mask, tris, max_tris


def render():
    edge_mask, tris, max_tris = tables()
    L = ["/* Generated by `python -m ngp_pl_amd.mc_tables` from cube topology; do not edit.",
         " * corner c = (c & 1, (c >> 1) & 1, (c >> 2) & 1); case = sum of 1 << c over inside corners.",
         " * edge e joins corners NGP_MC_EDGE_CORNERS[e][0] < [1]; it runs along axis e / 4 and is owned by corner [0].",
         " * Triangles are counter-clockwise seen from outside (the normal points from inside to outside). */",
         "#ifndef NGP_MC_TABLES_H", "#define NGP_MC_TABLES_H", "",
         "#define NGP_MC_MAX_TRIS %d" % max_tris, "",
         "/* storage class of the tables: device code defines it as __constant__ before including this header */",
         "#ifndef NGP_MC_STORAGE", "#define NGP_MC_STORAGE static const", "#endif", "",
         "NGP_MC_STORAGE unsigned char NGP_MC_EDGE_CORNERS[12][2] = {",
         "    " + ", ".join("{%d, %d}" % e for e in EDGES), "};", "",
         "NGP_MC_STORAGE unsigned short NGP_MC_EDGE_MASK[256] = {"]
    for r in range(0, 256, 16):
        L.append("    " + ", ".join("0x%03x" % m for m in edge_mask[r:r + 16]) + ",")
    L += ["};", "", "NGP_MC_STORAGE unsigned char NGP_MC_TRI_COUNT[256] = {"]
    for r in range(0, 256, 32):
        L.append("    " + ", ".join(str(len(t)) for t in tris[r:r + 32]) + ",")
    L += ["};", "", "NGP_MC_STORAGE signed char NGP_MC_TRIS[256][%d] = {" % (3 * max_tris)]
    for c in range(256):
        flat = [e for t in tris[c] for e in t] + [-1] * (3 * (max_tris - len(tris[c])))
        L.append("    {" + ", ".join(str(e) for e in flat) + "},")
    L += ["};", "", "#endif", ""]
    return "\n".join(L)


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        sys.exit(0 if open(HEADER).read() == text else 1)
    os.makedirs(os.path.dirname(HEADER), exist_ok=True)
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote", HEADER)
