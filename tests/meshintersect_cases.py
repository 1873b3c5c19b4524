"""The hand-built meshes of the intersection tests (tests/test_meshintersect_ref.py on the CPU, tests/test_gpu_meshintersect.py
on the GPU): numpy only.  HAND maps a name to (verts [V, 3] float64, faces [F, 3] int64, the pairs [(a, b, kind)] a self
run must report)."""
import numpy as np

import meshhole_cases

CROSSING, COPLANAR, UNCERTAIN = 1, 2, 3
NAN = float("nan")


def _mesh(verts, faces):
    return np.array(verts, np.float64), np.array(faces, np.int64)


def _fan():
    t = 2 * np.pi * np.arange(6) / 6
    verts = np.concatenate([[[0.0, 0.0, 0.0]], np.stack([np.cos(t), np.sin(t), np.zeros(6)], 1)])
    return verts, np.array([(0, 1 + i, 1 + (i + 1) % 6) for i in range(6)], np.int64)


BASE = [(-1, -1, 0), (1, -1, 0), (0, 1, 0)]                    # a triangle in the plane z = 0 around the origin
HAND = {
    # two triangles crossing like a plus
    "plus": (*_mesh(BASE + [(0.1, -0.3, -1), (0.1, -0.3, 1), (0.05, 0.3, 0.1)], [(0, 1, 2), (3, 4, 5)]),
             [(0, 1, CROSSING)]),
    # a corner of the second lies exactly in the face of the first
    "corner_in_face": (*_mesh(BASE + [(0, 0, 0), (0.3, 0.1, 1), (-0.2, 0.1, 1)], [(0, 1, 2), (3, 4, 5)]),
                       [(0, 1, UNCERTAIN)]),
    "coplanar_overlap": (*_mesh(BASE + [(0, 0, 0), (2, 0, 0), (1, 2, 0)], [(0, 1, 2), (3, 4, 5)]), [(0, 1, COPLANAR)]),
    # coplanar, the boxes overlap, the hypotenuse of the first separates them
    "coplanar_apart": (*_mesh([(0, 0, 0), (2, 0, 0), (0, 2, 0), (2, 2, 0), (2, 0.5, 0), (0.5, 2, 0)], [(0, 1, 2), (3, 4, 5)]),
                       []),
    # two faces over one edge, folded flat onto each other
    "flat_fold": (*_mesh([(0, 0, 0), (1, 0, 0), (0.5, 1, 0), (0.4, 0.8, 0)], [(0, 1, 2), (1, 0, 3)]), [(0, 1, COPLANAR)]),
    "flat_fan": (*_fan(), []),
    "flat_grid": (*meshhole_cases.grid(4, 3), []),
    # one shared vertex; the edge opposite to it in the second face pierces the first
    "vertex_pierce": (*_mesh([(0, 0, 0), (2, 0, 0), (0, 2, 0), (0.5, 0.5, -1), (0.6, 0.7, 1)], [(0, 1, 2), (0, 3, 4)]),
                      [(0, 1, CROSSING)]),
    # one shared vertex, the second face standing on the first's plane away from it
    "vertex_clear": (*_mesh([(0, 0, 0), (2, 0, 0), (0, 2, 0), (-0.5, -0.5, -1), (-0.6, -0.7, 1)], [(0, 1, 2), (0, 3, 4)]), []),
    # a corner of the second exactly in the plane of the first but outside it: the edges decide, nothing touches
    "corner_in_plane_outside": (*_mesh(BASE + [(0.9, 0.5, 0), (1.2, 0.6, 1), (0.7, 0.6, 1)], [(0, 1, 2), (3, 4, 5)]), []),
    # one shared vertex and an edge of the second lying in the plane of the first, outside it (the two halves of a flat
    # quad and a neighbour of one of them, as a mesher leaves them)
    "vertex_edge_in_plane": (*_mesh([(0, 0, 0), (1, 1, 0), (0, 1, 0), (0.3, -0.5, 0.7), (1, 0, 0)], [(0, 1, 2), (0, 3, 4)]), []),
    "duplicate_face": (*_mesh(BASE, [(0, 1, 2), (1, 2, 0), (2, 1, 0)]), []),
    # the plus with a third face that would cross the first had it no NaN vertex: absent
    "nan_vertex": (*_mesh(BASE + [(0.1, -0.3, -1), (0.1, -0.3, 1), (0.05, 0.3, 0.1), (0.2, -0.3, -1), (0.2, -0.3, 1),
                                  (NAN, 0.3, 0.1)], [(0, 1, 2), (3, 4, 5), (6, 7, 8)]), [(0, 1, CROSSING)]),
}


def _wavy(xs, ys):
    return 0.3 * np.sin(0.9 * xs + 0.2) * np.cos(0.7 * ys - 0.4) + 0.005 * xs * ys


def spiked_sheet():
    """a wavy 9 x 9 sheet (its own border of 36 edges stays open at max_edges=32) with two holes of 6 edges, each two
    quads left out, and a spike of two faces over a vertical ridge that stands through the first hole without touching
    the sheet -> (verts, faces, a rim vertex of the spiked hole, a rim vertex of the clear hole).  Wavy, because the
    three rim vertices on a side of such a hole in a flat sheet lie on one line: every minimum-area patch of it has a
    face of no area lying along the rim, which is a COPLANAR pair with the sheet's faces there in its own right."""
    verts, faces = meshhole_cases.grid(9, 9, skip_quads=[(3, 3), (4, 3), (2, 6), (3, 6)], height=_wavy)
    n = len(verts)
    spike = np.array([(3.7, 3.45, -1.0), (3.7, 3.45, 1.0), (4.4, 3.6, 0.2), (3.3, 3.7, -0.3)])
    verts = np.concatenate([verts, spike])
    faces = np.concatenate([faces, [(n, n + 1, n + 2), (n + 1, n, n + 3)]])
    return verts, faces, 3 * 10 + 3, 6 * 10 + 2
