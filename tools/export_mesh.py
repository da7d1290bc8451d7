#!/usr/bin/env python
"""Checkpoint -> isosurface mesh (the reference's --export_mesh, train.py:107-118), on the device.

    python tools/export_mesh.py ckpt.th out.ply [--time T] [--level L] [--grid G0 G1 G2] [--cap] [--normals] [--flip]
                                                [--world H W focal] [--color-view X Y Z] [--simplify K] [--with-static CKPT]
                                                [--texture Q [--texture-view normal]]

--time is required for a dynamic field (times run over [-1, 1]); --world maps the vertices of an ndc field to world space;
--color-view writes vertex colours: the field's rgb at the field-space vertices seen along the direction X Y Z (used as given);
--simplify K clusters the vertices K lattice cells wide (mean position, normal and colour per cluster; degenerate faces dropped);
--with-static CKPT: ckpt.th is the dynamic field and CKPT the static one, and the mesh is the whole scene's at --time: the
isosurface of the alpha the renderer composes from both, colours blended by the dynamic field's share;
--texture Q writes out.obj, out.mtl and out.png instead of a PLY: a texture atlas with squares of Q x Q texels, two faces to a
square, the field's colour per texel of the final (simplified) mesh, seen along --color-view (default 0 0 1) or, with
--texture-view normal, along minus each face's normal."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("ckpt")
    ap.add_argument("ply")
    ap.add_argument("--time", type=float, default=None)
    ap.add_argument("--level", type=float, default=0.005)
    ap.add_argument("--grid", type=int, nargs=3, default=None, metavar=("G0", "G1", "G2"))
    ap.add_argument("--cap", action="store_true")
    ap.add_argument("--normals", action="store_true")
    ap.add_argument("--flip", action="store_true")
    ap.add_argument("--world", type=float, nargs=3, default=None, metavar=("H", "W", "focal"))
    ap.add_argument("--color-view", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    ap.add_argument("--simplify", type=int, default=None, metavar="K")
    ap.add_argument("--with-static", default=None, metavar="CKPT")
    ap.add_argument("--texture", type=int, default=None, metavar="Q")
    ap.add_argument("--texture-view", choices=["normal"], default=None)
    a = ap.parse_args()
    import rodynrf
    kw = dict(cap=a.cap, normals=a.normals, flip=a.flip)
    if a.simplify is not None:
        kw.update(simplify=a.simplify)
    if a.world is not None:
        kw.update(space="world", H=a.world[0], W=a.world[1], focal=a.world[2])
    if a.color_view is not None:
        kw.update(color_view=tuple(a.color_view))
    if a.with_static is not None:
        kw.update(static=a.with_static)
    if a.texture_view is not None and (a.texture is None or a.color_view is not None):
        ap.error("--texture-view normal goes with --texture and without --color-view")
    if a.texture is not None:
        kw.update(texture=a.texture)
        if a.texture_view is not None:
            kw.update(color_view=a.texture_view)
    out = rodynrf.export_mesh(a.ckpt, a.ply, t=a.time, level=a.level, gridSize=a.grid, **kw)
    where = a.ply if a.texture is None else ", ".join(rodynrf.mesh._obj_paths(a.ply))   # the three files write_obj wrote
    print(f"{where}: {out[0].shape[0]} vertices, {out[1].shape[0]} faces")


if __name__ == "__main__":
    main()
