"""Plain numpy / Python restatement of libngp_meshfilter.so (include/ngp_meshfilter.h): connected components of an indexed
triangle mesh by a sequential union-find over the faces, labels by smallest vertex index, faces per component, the selection
rules of ngp_pl_amd.mesh.filter_components and the order-preserving compaction.  Test infrastructure only."""
import numpy as np


def vertex_labels(faces, n_vertices):
    """(V,) i32: the smallest vertex index of each vertex's component.  Union-find with path halving, the larger root hooked
    under the smaller, so a root is the minimum of its tree."""
    parent = list(range(n_vertices))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        for u in (b, c):
            ra, ru = find(a), find(u)
            if ra < ru:
                parent[ru] = ra
            elif ru < ra:
                parent[ra] = ru
    return np.array([find(v) for v in range(n_vertices)], np.int32).reshape(n_vertices)


class Components:
    def __init__(self, faces, n_vertices):
        faces = np.asarray(faces, np.int32).reshape(-1, 3)
        self.vertex_label = vertex_labels(faces, n_vertices)
        self.face_label = self.vertex_label[faces[:, 0]].astype(np.int32)
        self.component_faces = np.bincount(self.face_label, minlength=n_vertices).astype(np.int32)    # at the label's index
        self.labels = np.nonzero(self.component_faces)[0].astype(np.int32)                          # ascending
        self.faces_per_component = self.component_faces[self.labels].astype(np.int64)
        self.n_components = len(self.labels)


def select(comps, keep_largest=None, min_faces=None):
    """Bool (C,) over comps.labels: at least min_faces faces, and among the keep_largest components with the most faces, ties to
    the smaller label."""
    sel = np.ones(comps.n_components, bool)
    if min_faces is not None:
        sel &= comps.faces_per_component >= min_faces
    if keep_largest is not None:
        order = np.lexsort((comps.labels, -comps.faces_per_component))         # most faces first, then the smaller label
        top = np.zeros(comps.n_components, bool)
        top[order[:keep_largest]] = True
        sel &= top
    return sel


def filter_components(vertices, faces, normals=None, colors=None, keep_largest=None, min_faces=None):
    """-> vertices', faces', normals', colors': kept faces (label selected) and the vertices they reference, in the input's
    order, faces re-indexed."""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    n_v = len(vertices)
    comps = Components(faces, n_v)
    keep = np.zeros(n_v, bool)
    keep[comps.labels[select(comps, keep_largest, min_faces)]] = True
    fkeep = keep[comps.face_label]
    kept_faces = faces[fkeep]
    used = np.zeros(n_v, bool)
    used[kept_faces.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    new_faces = remap[kept_faces].astype(np.int32).reshape(-1, 3)
    pick = lambda a: None if a is None else np.asarray(a)[used]
    return pick(vertices), new_faces, pick(normals), pick(colors)
