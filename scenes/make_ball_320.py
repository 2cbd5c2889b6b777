"""Writes scenes/ball_320.obj: an icosphere of 320 triangles (an icosahedron subdivided twice) of radius 0.5 about the origin -- the
size of the format's `sphere` -- with one `vn` per vertex, the analytic normal.  Seedless and deterministic:

    python scenes/make_ball_320.py
"""
import math
import os


def icosphere(levels):
    t = (1.0 + math.sqrt(5.0)) / 2.0
    raw = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
           (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    verts = []
    for v in raw:
        n = math.sqrt(sum(c * c for c in v))
        verts.append(tuple(c / n for c in v))
    # counter-clockwise seen from outside
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = tuple((verts[a][k] + verts[b][k]) / 2.0 for k in range(3))
                n = math.sqrt(sum(c * c for c in m))
                verts.append(tuple(c / n for c in m))
                mid[key] = len(verts) - 1
            return mid[key]

        nxt = []
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nxt
    return verts, faces


def main():
    verts, faces = icosphere(2)
    assert len(faces) == 320 and len(verts) == 162
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ball_320.obj")
    with open(path, "w") as f:
        f.write("# icosphere, 162 vertices, 320 triangles, radius 0.5; written by make_ball_320.py\n")
        for v in verts:
            f.write("v %.9g %.9g %.9g\n" % tuple(0.5 * c for c in v))
        for v in verts:
            f.write("vn %.9g %.9g %.9g\n" % v)
        for a, b, c in faces:
            f.write("f %d//%d %d//%d %d//%d\n" % (a + 1, a + 1, b + 1, b + 1, c + 1, c + 1))


if __name__ == "__main__":
    main()
