"""Small synthetic scenes for the edge-case tests, written with the Veach generator's OBJ writer
(scenes/gen_veach_mis.py): a scene without lights, a dense light panel (more than 4096 candidates
per shading point: the sequential batch-search path) and a very finely tessellated sphere light
(N_L > 7680: the LDS-queue prep variant, no root cache)."""
import math
import os
import sys

from conftest import ROOT

sys.path.insert(0, str(ROOT / "scenes"))
import gen_veach_mis as gv  # noqa: E402


def _write(outdir, name, obj, mtls, lights, cam, fovy="20.1143"):
    os.makedirs(outdir, exist_ok=True)
    obj.write(os.path.join(outdir, name + ".obj"), name + ".mtl")
    with open(os.path.join(outdir, name + ".mtl"), "w", newline="\n") as f:
        for m, kd, ks, ns in mtls:
            f.write("newmtl %s\nKd %.6f %.6f %.6f\nKs %.6f %.6f %.6f\nNs %.6f\n\n" % ((m,) + kd + ks + (ns,)))
    with open(os.path.join(outdir, name + ".xml"), "w", newline="\n") as f:
        eye, look = cam
        f.write('<camera type="perspective" width="16" height="12" fovy="%s">\n'
                '\t<eye x="%r" y="%r" z="%r"/>\n\t<lookat x="%r" y="%r" z="%r"/>\n'
                '\t<up x="0.0" y="1.0" z="0.0"/>\n</camera>\n' % ((fovy,) + eye + look))
        for m, rad in lights:
            f.write('<light mtlname="%s" radiance="%.6f,%.6f,%.6f"/>\n' % ((m,) + rad))
    return os.path.join(outdir, name + ".obj"), os.path.join(outdir, name + ".xml")


def _floor(obj, mtls):
    obj.box("floor", "floor", (0.0, -0.1, 0.0), [((1.0, 0.0, 0.0), 4.0), ((0.0, 1.0, 0.0), 0.1), ((0.0, 0.0, 1.0), 4.0)])
    obj.box("block", "glossy", (0.5, 0.4, 0.3), [((1.0, 0.0, 0.0), 0.4), ((0.0, 1.0, 0.0), 0.4), ((0.0, 0.0, 1.0), 0.4)])
    mtls += [("floor", (0.5, 0.5, 0.5), (0.0, 0.0, 0.0), 1.0), ("glossy", (0.1, 0.1, 0.1), (0.4, 0.4, 0.4), 50.0)]


CAM = ((0.0, 3.0, 9.0), (0.0, 0.5, 0.0))


def no_lights(outdir):
    obj, mtls = gv.Obj(), []
    _floor(obj, mtls)
    return _write(outdir, "nolight", obj, mtls, [], CAM)


def light_panel(outdir, nx=60, nz=60):
    """a downward-facing light panel of nx x nz quads (2 nx nz triangles) above the floor"""
    obj, mtls = gv.Obj(), []
    _floor(obj, mtls)
    faces = []
    n = obj.normal((0.0, -1.0, 0.0))
    y, x0, x1, z0, z1 = 2.5, -1.5, 1.5, -1.5, 1.5
    for i in range(nx):
        for k in range(nz):
            xa, xb = x0 + (x1 - x0) * i / nx, x0 + (x1 - x0) * (i + 1) / nx
            za, zb = z0 + (z1 - z0) * k / nz, z0 + (z1 - z0) * (k + 1) / nz
            a, b = obj.vert((xa, y, za)), obj.vert((xb, y, za))
            c, d = obj.vert((xb, y, zb)), obj.vert((xa, y, zb))
            faces.append(((a, n), (b, n), (c, n)))  # (b-a) x (c-a) = -y: faces the floor
            faces.append(((a, n), (c, n), (d, n)))
    obj.groups.append(("panel", "panel", faces))
    mtls.append(("panel", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0))
    return _write(outdir, "panel", obj, mtls, [("panel", (2.0, 2.0, 2.0))], CAM)


def dense_sphere(outdir, nseg=120, nring=60):
    obj, mtls = gv.Obj(), []
    _floor(obj, mtls)
    obj.sphere("bulb", "bulb", (-0.8, 1.6, 0.0), 0.5, nseg, nring)
    mtls.append(("bulb", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0))
    return _write(outdir, "bulb", obj, mtls, [("bulb", (20.0, 18.0, 15.0))], CAM)


def occluded_room(outdir):
    """A closed room (inward faces of six wall slabs) with a down-facing ceiling lamp and an up-facing
    floor lamp, each hidden behind a close, wider cap: a light sample from almost any point hits a
    cap, and the cap's outer side faces the OTHER lamp, so an MIS node has two non-emitter children
    with probability ~0.6 each -- a supercritical tree (~1.2 children per node, main.cpp:455-491)
    whose generations outgrow any fixed wavefront queue."""
    obj, mtls = gv.Obj(), []
    X, Y, Z, T = 2.0, 3.0, 2.0, 0.1  # room half extents (y from 0 to Y), wall thickness
    ex, ey, ez = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    walls = [((0.0, -T, 0.0), [(ex, X + T), (ey, T), (ez, Z + T)]),
             ((0.0, Y + T, 0.0), [(ex, X + T), (ey, T), (ez, Z + T)]),
             ((-X - T, Y / 2, 0.0), [(ex, T), (ey, Y / 2), (ez, Z + T)]),
             ((X + T, Y / 2, 0.0), [(ex, T), (ey, Y / 2), (ez, Z + T)]),
             ((0.0, Y / 2, -Z - T), [(ex, X), (ey, Y / 2), (ez, T)]),
             ((0.0, Y / 2, Z + T), [(ex, X), (ey, Y / 2), (ez, T)])]
    for k, (c, axes) in enumerate(walls):
        obj.box("wall%d" % k, "wall", c, axes)
    faces = []
    for x0, y, ny in ((-0.8, Y - 0.05, -1.0), (0.8, 0.05, 1.0)):  # lamp quads: 0.4 x 0.4
        n = obj.normal((0.0, ny, 0.0))
        q = [obj.vert((x0 + sx * 0.2, y, sz * 0.2)) for sx, sz in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        tri = [(q[0], q[2], q[1]), (q[0], q[3], q[2])] if ny < 0 else [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
        tri = [t if ny > 0 else t for t in tri]
        faces += [tuple((v, n) for v in t) for t in tri]
        obj.box("cap%d" % len(faces), "wall", (x0, y + 0.1 * ny, 0.0), [(ex, 0.35), (ey, 0.01), (ez, 0.35)])
    obj.groups.append(("lamp", "lamp", faces))
    mtls += [("wall", (0.7, 0.7, 0.7), (0.0, 0.0, 0.0), 1.0), ("lamp", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0)]
    return _write(outdir, "room", obj, mtls, [("lamp", (5.0, 5.0, 5.0))], ((0.0, 1.5, 1.8), (0.0, 0.4, 0.0)))


# ---- exact-pick stress scenes (the band + literal fallback beyond the stand-in) ----

def sphere_mix(outdir):
    """Four sphere lights of 8x4, 16x8, 32x16 and 64x32 segments (48 + 224 + 960 + 3968 = 5200 light
    triangles: more than 4096, so roots take the wave-per-root k_prep_pick), different radii, distances
    and radiances over the floor and a glossy block."""
    obj, mtls = gv.Obj(), []
    _floor(obj, mtls)
    lights = []
    for k, (seg, ring, c, r, rad) in enumerate([(8, 4, (-1.6, 1.9, -1.0), 0.35, (3.0, 2.0, 1.0)),
                                                (16, 8, (1.6, 2.1, -1.2), 0.2, (9.0, 9.0, 12.0)),
                                                (32, 16, (0.0, 2.6, -1.6), 0.5, (2.0, 2.5, 2.0)),
                                                (64, 32, (-0.3, 1.5, 1.4), 0.3, (4.0, 3.0, 3.0))]):
        name = "sph%d" % k
        obj.sphere(name, name, c, r, seg, ring)
        mtls.append((name, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0))
        lights.append((name, rad))
    return _write(outdir, "sphmix", obj, mtls, lights, CAM)


def _blinds(obj, xs, strips):
    """the faces of vertical light blinds in the planes x = xk (two thin layers each, facing +x and -x), `strips` long
    thin quads high"""
    faces = []
    for xk in xs:
        for side in (1.0, -1.0):  # two thin layers facing +x and -x
            x = xk + 0.002 * side
            n = obj.normal((side, 0.0, 0.0))
            for s in range(strips):
                y0, y1 = 0.3 + 1.5 * s / strips, 0.3 + 1.5 * (s + 1) / strips
                a, b = obj.vert((x, y0, -1.5)), obj.vert((x, y0, 1.5))
                c, d = obj.vert((x, y1, 1.5)), obj.vert((x, y1, -1.5))
                tri = [(a, b, c), (a, c, d)]
                if side < 0:
                    tri = [(a, c, b), (a, d, c)]
                faces += [tuple((v, n) for v in t) for t in tri]
    return faces


def _tiny_lights(obj, mtls, lights, radii, places):
    """8x4 sphere lights "tinyNN" of every radius at every (distance above the floor, azimuth)"""
    k = 0
    for r in radii:
        for dist, az in places:
            name = "tiny%02d" % k
            c = (dist * 0.3 * math.cos(az), dist, dist * 0.3 * math.sin(az))
            obj.sphere(name, name, c, r, 8, 4)
            mtls.append((name, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0))
            lights.append((name, (4000.0, 3000.0, 2000.0)))
            k += 1


def slivers(outdir, strips=24):
    """Lights seen nearly edge-on from the floor: vertical light blinds (planes x = const, split into
    long thin triangles) standing on the floor region, whose planes pass through the floor points next
    to them -- their spherical triangles are slivers (one vertex angle near pi), where the reference's
    alpha + beta + gamma - pi is decided by the last bits of its acos; plus a panel tilted 2 degrees
    off the vertical (near-grazing for the points below it)."""
    obj, mtls = gv.Obj(), []
    _floor(obj, mtls)
    obj.groups.append(("blinds", "blinds", _blinds(obj, (-1.2, -0.4, 0.4, 1.2), strips)))
    faces = []
    t = math.radians(2.0)
    n = obj.normal((math.cos(t), math.sin(t), 0.0))
    for s in range(40):  # tilted panel of 80 thin triangles near x = 2.2
        z0, z1 = -1.5 + 3.0 * s / 40, -1.5 + 3.0 * (s + 1) / 40
        p = [(2.2 - 1.6 * math.sin(t) * h, 0.2 + 1.6 * math.cos(t) * h, z) for h, z in ((0, z0), (0, z1), (1, z1), (1, z0))]
        q = [obj.vert(v) for v in p]
        faces += [((q[0], n), (q[2], n), (q[1], n)), ((q[0], n), (q[3], n), (q[2], n))]
    obj.groups.append(("tilt", "tilt", faces))
    mtls += [("blinds", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0), ("tilt", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0)]
    return _write(outdir, "slivers", obj, mtls, [("blinds", (4.0, 4.0, 4.0)), ("tilt", (6.0, 5.0, 4.0))], CAM)


def tiny_far(outdir):
    """Distant tiny lights: 8x4 spheres of radius 1e-2, 1e-3, 1e-4 and 1e-6 at distances 20-90 above the
    floor, plus one ordinary light.  Their spherical triangles span ~1e-2 .. 1e-8 rad: the reference's
    alpha + beta + gamma - pi is mostly its own rounding there (the unit vectors' rounding amplified by
    distance / edge), and the edge-length culls (< 1e-8 rad, Mylight.cpp:379-382) fire on the smallest."""
    obj, mtls = gv.Obj(), []
    _floor(obj, mtls)
    lights = []
    _tiny_lights(obj, mtls, lights, (1e-2, 1e-3, 1e-4, 1e-6), ((20.0, 0.3), (45.0, 1.9), (90.0, 4.0)))
    obj.sphere("lamp", "lamp", (1.2, 2.2, -0.8), 0.25, 16, 8)
    mtls.append(("lamp", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0))
    lights.append(("lamp", (5.0, 5.0, 5.0)))
    return _write(outdir, "tinyfar", obj, mtls, lights, CAM)


def light_soup(outdir, n=1500, seed=3):
    """n unrelated light triangles (round 6): random positions 0.3-40 units above / around the floor, random
    orientations, sizes spanning 1e-4 .. 1 (log-uniform) and shapes from equilateral to slivers (one vertex pulled
    to within 1e-3 of the opposite edge), one of five radiances each -- no tessellated sphere, no shared edges, so
    the spherical triangles of a shading point cover every size, aspect and viewing angle the band must bound"""
    import random
    rng = random.Random(seed)
    obj, mtls = gv.Obj(), []
    _floor(obj, mtls)
    groups = {k: [] for k in range(5)}
    for _ in range(n):
        c = (rng.uniform(-8.0, 8.0), 0.3 + 40.0 * rng.random() ** 2, rng.uniform(-8.0, 8.0))
        size = 10.0 ** rng.uniform(-4.0, 0.0)
        u = gv.norm((rng.gauss(0, 1), rng.gauss(0, 1), rng.gauss(0, 1)))
        w = gv.norm(gv.cross(u, gv.norm((rng.gauss(0, 1), rng.gauss(0, 1), rng.gauss(0, 1)))))
        a = gv.add(c, gv.mul(u, -size))
        b = gv.add(c, gv.mul(u, size))
        h = size * (1e-3 if rng.random() < 0.2 else rng.uniform(0.2, 1.7))
        d = gv.add(gv.add(c, gv.mul(u, size * rng.uniform(-0.9, 0.9))), gv.mul(w, h))
        nrm = gv.norm(gv.cross(gv.sub(b, a), gv.sub(d, a)))
        ni = obj.normal(nrm)
        groups[rng.randrange(5)].append(((obj.vert(a), ni), (obj.vert(b), ni), (obj.vert(d), ni)))
    lights = []
    for k, faces in groups.items():
        name = "soup%d" % k
        obj.groups.append((name, name, faces))
        mtls.append((name, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0))
        lights.append((name, (3.0 * (k + 1), 2.0 * (k + 1), 1.0 * (k + 1))))
    return _write(outdir, "soup", obj, mtls, lights, CAM)


STRESS = {"sphmix": (sphere_mix, 5200), "slivers": (slivers, 8 * 24 * 2 + 80), "tinyfar": (tiny_far, 12 * 48 + 224),
          "dense": (dense_sphere, 14160), "soup": (light_soup, 1500)}


def needles(outdir, n=70000, seed=7, length=1.0):
    """n thin random triangles ("needles", up to `length` long) in a 10-unit box in every direction, plus the floor:
    nearly every object split of such a tree overlaps, so a >= 65 536-triangle build wants far more spatial-split
    duplicates than its budget (bvh.cpp MCPT_BVH_SPATIAL_BUDGET) allows -- the budget-exhausting case of the
    builder's determinism test"""
    import random
    rng = random.Random(seed)
    obj, mtls = gv.Obj(), []
    _floor(obj, mtls)
    ni = obj.normal((0.0, 1.0, 0.0))
    faces = []
    for _ in range(n):
        a = tuple(rng.uniform(-5.0, 5.0) for _ in range(3))
        b = tuple(min(5.0, max(-5.0, x + rng.uniform(-length, length))) for x in a)
        c = tuple(x + rng.uniform(-0.02, 0.02) for x in a)
        faces.append(((obj.vert(a), ni), (obj.vert(b), ni), (obj.vert(c), ni)))
    obj.groups.append(("needles", "floor", faces))
    return _write(outdir, "needles", obj, mtls, [], CAM)


# ---- material swatch: the Phong material classes the other scenes never render (tests/test_swatch.py) ----
SWATCH_TILES = [  # (name, Kd, Ks, Ns): the classes of tests/phonggen.py that a frame can show (no black, no Ns < 0)
    ("diffuse", (0.5, 0.5, 0.5), (0.0, 0.0, 0.0), 1.0),
    ("specular", (0.0, 0.0, 0.0), (0.5, 0.5, 0.5), 50.0),
    ("plates", (0.07, 0.09, 0.13), (0.1, 0.2, 0.3), 120.0),
    ("kszero", (0.2, 0.2, 0.2), (0.3, 0.0, 0.2), 50.0),
    ("tinykd", (1e-6, 1e-6, 1e-6), (0.5, 0.5, 0.5), 50.0),
    ("ns0", (0.07, 0.09, 0.13), (0.1, 0.2, 0.3), 0.0),
    ("nshalf", (0.07, 0.09, 0.13), (0.1, 0.2, 0.3), 0.5),
    ("ns1", (0.07, 0.09, 0.13), (0.1, 0.2, 0.3), 1.0),
    ("ns5000", (0.07, 0.09, 0.13), (0.1, 0.2, 0.3), 5000.0),
    ("spec1e6", (0.0, 0.0, 0.0), (0.5, 0.5, 0.5), 1e6),
    ("ns2e6", (0.07, 0.09, 0.13), (0.1, 0.2, 0.3), 2e6),
    ("diff1e6", (0.5, 0.5, 0.5), (0.0, 0.0, 0.0), 1e6),
]
SWATCH_SLABS = [("slab_px", (0.5, 0.5, 0.5), (0.0, 0.0, 0.0), 1.0), ("slab_nx", (0.0, 0.0, 0.0), (0.5, 0.5, 0.5), 50.0)]
# the reference takes tan(fovy / 360) of the XML's fovy (main.cpp's camera): 120 gives a half angle of 19 degrees
SWATCH_CAM, SWATCH_FOVY = ((0.0, 4.0, 3.0), (0.0, 0.3, 0.0)), "120.0"


def material_swatch(outdir):
    """A 4 x 3 grid of unit tiles, one Phong material class each (SWATCH_TILES), between two upright slabs whose large
    inner faces have the normals exactly +x (diffuse) and -x (specular only), under a 16 x 8 sphere light (224
    triangles) and a down-facing light quad: 226 lights, so the main prep path, the root cache and the exact fallback
    run.  The tiles abut, and the slabs close the grid's x ends from below the tiles to above them: every -x-facing
    side of a material with a diffuse part (the reference's cosine-lobe frame for n = -e_x exactly is 0 / 0, a NaN
    direction) is either covered by its neighbour or, on the +x slab's outer side, faces nothing a ray can leave
    from.  The -x slab has Kd = 0: its cosine lobe is picked for u0 == 0 only."""
    obj, mtls = gv.Obj(), []
    ex, ey, ez = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    for k, (name, kd, ks, ns) in enumerate(SWATCH_TILES):
        i, j = k % 4, k // 4
        obj.box("tile_" + name, name, (i - 1.5, -0.1, j - 1.0), [(ex, 0.5), (ey, 0.1), (ez, 0.5)])
        mtls.append((name, kd, ks, ns))
    for (name, kd, ks, ns), x in zip(SWATCH_SLABS, (-2.125, 2.125)):  # inner faces at x = -2 and x = 2 exactly
        obj.box(name, name, (x, 1.0, 0.0), [(ex, 0.125), (ey, 1.5), (ez, 1.5)])
        mtls.append((name, kd, ks, ns))
    obj.sphere("bulb", "bulb", (-0.4, 2.6, -0.3), 0.35, 16, 8)
    n = obj.normal((0.0, -1.0, 0.0))
    q = [obj.vert(p) for p in ((0.3, 3.2, 0.2), (1.3, 3.2, 0.2), (1.3, 3.2, 1.2), (0.3, 3.2, 1.2))]
    obj.groups.append(("quad", "quad", [((q[0], n), (q[1], n), (q[2], n)), ((q[0], n), (q[2], n), (q[3], n))]))
    mtls += [("bulb", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0), ("quad", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0)]
    return _write(outdir, "swatch", obj, mtls, [("bulb", (20.0, 18.0, 15.0)), ("quad", (6.0, 7.0, 8.0))], SWATCH_CAM,
                  SWATCH_FOVY)


def swatch_owners(oscene, cam):
    """per pixel of the oracle's primary hits: the material index (-1: no hit) and whether the facet's normal is
    exactly +-e_x; plus the material names in the MTL's order"""
    import numpy as np
    from oracle import pyoracle as po

    _, mat, _, un = oscene.facets()
    owner = np.full(cam.width * cam.height, -1)
    xface = np.zeros(cam.width * cam.height, bool)
    for i in range(cam.height):  # the oracle's pixel order: row i, column j, pixel i * width + j
        for j in range(cam.width):
            e, d = po.camera_ray(cam, i, j)
            f, _ = oscene.closest_hit(e, d)
            if f >= 0:
                owner[i * cam.width + j] = mat[f]
                xface[i * cam.width + j] = abs(un[f][0]) == 1.0 and un[f][1] == 0.0 and un[f][2] == 0.0
    return owner, xface


# ---- traversal stress: a cluster that can sit far from the origin, and the ray families aimed at it ----
# (tests/test_traversal_stress.py, tests/test_traversal_stress_cpu.py)
class _ObjExact(gv.Obj):
    """gv.Obj whose vertices are written with every digit (the float32 the loader makes of them is then the
    float32 of the double computed here, at any offset and scale)"""

    def write(self, path, mtllib):
        with open(path, "w", newline="\n") as f:
            f.write("mtllib %s\n" % mtllib)
            for p in self.v:
                f.write("v %.17g %.17g %.17g\n" % p)
            for n in self.vn:
                f.write("vn %.9g %.9g %.9g\n" % n)
            for name, mtl, faces in self.groups:
                f.write("o %s\nusemtl %s\n" % (name, mtl))
                for tri in faces:
                    f.write("f %s\n" % " ".join("%d//%d" % vn for vn in tri))


STRESS_LATTICE = 64  # lattice coordinates: multiples of scale / 64
# facets in file order: (group, number of triangles)
STRESS_GROUPS = (("random", 1400), ("lattice", 500), ("coincident", 64), ("degenerate", 8), ("anchor", 2), ("floor", 2),
                 ("light", 2))


def stress_ranges():
    """group -> (first facet, end facet) of ray_stress's scene"""
    out, at = {}, 0
    for name, n in STRESS_GROUPS:
        out[name] = (at, at + n)
        at += n
    return out


def ray_stress(outdir, offset=(0, 0, 0), scale=1.0, seed=5):
    """About 2 000 triangles in a box of extent `scale` whose corner sits at offset * scale (offset in extents): a unit
    cluster u in [0, 1]^3 written at scale * (u + offset).  In file order (STRESS_GROUPS):
      * 1 400 random triangles, edge lengths log-uniform in 1e-4 .. 1e-1 of the extent;
      * 250 axis-aligned quads on lattice coordinates (multiples of scale / 64, 1 .. 8 cells wide): shared planes, flat
        boxes, edges lying on box faces; the quads in x-planes have no diffuse part (the reference's cosine-lobe frame
        is 0 / 0 for a normal of exactly -e_x);
      * 32 pairs of coincident triangles: 16 pairs on the lattice (y- and z-planes), 16 of random orientation, the odd
        pairs' second copy with its vertices rotated (same triangle, another operation order);
      * 8 zero-area facets: 4 with collinear vertices, 4 with a repeated vertex;
      * an anchor quad across the bottom of the box (y = 0), a floor just above it (y = 2 / 64) and one light quad (y = 1, 0.6 extents wide, facing down)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    off = np.asarray(offset, np.float64)
    obj, L = _ObjExact(), STRESS_LATTICE

    def place(u):
        return tuple(float(x) for x in scale * (np.asarray(u, np.float64) + off))

    def tri(faces, pts, n):
        ni = obj.normal(tuple(float(x) for x in n))
        faces.append(tuple((obj.vert(place(p)), ni) for p in pts))

    def geo_normal(p):
        n = np.cross(np.subtract(p[1], p[0]), np.subtract(p[2], p[0]))
        l = np.linalg.norm(n)
        return n / l if l > 0 else np.array([0.0, 1.0, 0.0])

    def random_tri(size):
        m = 0.02 + size  # the triangle reaches at most `size` from c: it stays inside the unit box
        c = rng.uniform(m, 1.0 - m, 3)
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        w = np.cross(u, rng.normal(size=3))
        w /= np.linalg.norm(w)
        return [c - 0.5 * size * u, c + 0.5 * size * u, c + size * (rng.uniform(-0.4, 0.4) * u + rng.uniform(0.3, 0.9) * w)]

    def lattice_pts(axis, p, i, j, w, h):
        o = [k for k in range(3) if k != axis]
        pts = []
        for a, b in ((i, j), (i + w, j), (i + w, j + h), (i, j + h)):
            q = [0.0, 0.0, 0.0]
            q[axis], q[o[0]], q[o[1]] = p / L, a / L, b / L
            pts.append(q)
        return pts

    groups = {name: [] for name, _ in STRESS_GROUPS}
    for _ in range(1400):
        p = random_tri(10.0 ** rng.uniform(-4.0, -1.0))
        tri(groups["random"], p, geo_normal(p))
    lat_x, lat_yz = [], []
    for k in range(250):
        axis = k % 3
        w, h = (int(x) for x in rng.choice([1, 2, 4, 8], 2))
        q = lattice_pts(axis, int(rng.integers(6, L - 5)), int(rng.integers(2, L - 2 - w)), int(rng.integers(2, L - 2 - h)), w, h)
        n = geo_normal(q[:3])
        for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
            tri(lat_x if axis == 0 else lat_yz, t, n)
    # the loader keeps file order inside a group; x-plane quads come first ("mirror" has no diffuse part)
    for k in range(32):
        if k < 16:
            q = lattice_pts(1 + k % 2, int(rng.integers(6, L - 5)), int(rng.integers(2, L - 12)), int(rng.integers(2, L - 12)),
                            int(rng.integers(4, 9)), int(rng.integers(4, 9)))
            p = [q[0], q[1], q[3]]
        else:
            p = random_tri(rng.uniform(0.05, 0.2))
        n = geo_normal(p)
        tri(groups["coincident"], p, n)
        tri(groups["coincident"], p[1:] + p[:1] if k % 2 else p, n)
    for k in range(8):
        p = random_tri(0.05)
        p = [p[0], p[1], 0.5 * (np.asarray(p[0]) + p[1])] if k < 4 else [p[0], p[0], p[1]]
        tri(groups["degenerate"], p, (0.0, 1.0, 0.0))
    # the floor is not the box's lowest face: the reference's grid loses rays that start on a minimum face of its box
    # (its "crack"), and with them the oracle's frame; the anchor quad below spans the box and is seen from below only
    for name, y, a, b in (("anchor", 0.0, 0.0, 1.0), ("floor", 2.0 / L, 1.0 / L, 1.0 - 1.0 / L)):
        fl = [(a, y, a), (a, y, b), (b, y, b), (b, y, a)]  # (b - a) x (c - a) = +y
        for t in ((fl[0], fl[1], fl[2]), (fl[0], fl[2], fl[3])):
            tri(groups[name], t, (0.0, 1.0, 0.0))
    lq = [(0.2, 1.0, 0.2), (0.8, 1.0, 0.2), (0.8, 1.0, 0.8), (0.2, 1.0, 0.8)]  # faces the floor
    for t in ((lq[0], lq[1], lq[2]), (lq[0], lq[2], lq[3])):
        tri(groups["light"], t, (0.0, -1.0, 0.0))
    assert len(lat_x) + len(lat_yz) == 500
    obj.groups.append(("random", "diffuse", groups["random"]))
    obj.groups.append(("lattice_x", "mirror", lat_x))
    obj.groups.append(("lattice_yz", "glossy", lat_yz))
    for name in ("coincident", "degenerate", "anchor", "floor"):
        obj.groups.append((name, "diffuse", groups[name]))
    obj.groups.append(("light", "lamp", groups["light"]))
    mtls = [("diffuse", (0.5, 0.5, 0.5), (0.0, 0.0, 0.0), 1.0), ("mirror", (0.0, 0.0, 0.0), (0.5, 0.5, 0.5), 50.0),
            ("glossy", (0.1, 0.1, 0.1), (0.4, 0.4, 0.4), 50.0), ("lamp", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0)]
    cam = (place((0.5, 0.95, 3.0)), place((0.5, 0.2, 0.5)))
    # from 2.6 extents in front of the box, looking down at the floor through the cluster
    return _write(outdir, "stress", obj, mtls, [("lamp", (40.0, 36.0, 30.0))], cam, "60.0")


STRESS_FAMILIES = ("aimed", "secondary", "axis", "far", "scaled")
STRESS_RAYS = 4096 + 37  # a partial block


def stress_rays(arrays, family, seed=11):
    """(origins, directions, excluded facet) of one ray family over the arrays of a loaded ray_stress scene (the
    float32 positions the library holds: targets are points of THOSE triangles, computed in double):
      aimed      at vertices, edge points and interior points, and points a relative 1e-15 / 1e-12 / 1e-9 off them,
                 from origins inside the box 0.05 extents from the target;
      secondary  origins on a facet (excluded), directions cosine-distributed about either side's normal -- and, for
                 every other ray, aimed at another facet's vertex / edge / interior point as a shadow ray is;
      axis       one or two direction components exactly 0.0 or -0.0, every origin coordinate a lattice coordinate,
                 along lattice lines and inside lattice planes, at lattice vertices, edge and interior points;
      far        the aimed targets from 1e2 and 1e4 extents outside the box;
      scaled     the aimed rays with the direction multiplied by 1e-3 (first half) and 1e3 (second half).
    The last ray of every family has a NaN direction."""
    import numpy as np
    rng = np.random.default_rng(seed + (0 if family == "scaled" else STRESS_FAMILIES.index(family)))
    n, R = STRESS_RAYS, stress_ranges()
    P = arrays["positions"].astype(np.float64).reshape(-1, 3, 3)
    lo, hi = P.reshape(-1, 3).min(axis=0), P.reshape(-1, 3).max(axis=0)
    ext = float((hi - lo).max())
    cr = np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
    hittable = cr >= 4e-8  # |detA| = |ab x ac| cos >= 1e-8 from most directions of a unit ray

    def ids(name, only=hittable):
        a, b = R[name]
        f = np.arange(a, b)
        return f[only[a:b]]

    rand_ok, lat, coin = ids("random"), ids("lattice"), ids("coincident")
    if len(rand_ok) < 50:
        rand_ok = lat

    def pick_tris(m, p_coin=0.08, lattice_only=False):
        u = rng.random(m)
        t = rand_ok[rng.integers(0, len(rand_ok), m)]
        t = np.where(u < 0.35, lat[rng.integers(0, len(lat), m)], t)
        if lattice_only:
            lc = coin[coin < R["coincident"][0] + 32]
            t = lat[rng.integers(0, len(lat), m)]
            return np.where(u < p_coin, lc[rng.integers(0, len(lc), m)], t)
        t = np.where(u < p_coin, coin[rng.integers(0, len(coin), m)], t)
        return np.where(u > 0.97, rng.integers(R["floor"][0], R["light"][1], m), t)

    def targets(tri, perturb=True, eps=(0.0, 0.0, 1e-15, -1e-15, 1e-12, -1e-12, 1e-9, -1e-9)):
        m = len(tri)
        kind = rng.integers(0, 3, m)
        w = rng.random((m, 3))
        w[kind == 0] = np.eye(3)[rng.integers(0, 3, int((kind == 0).sum()))]  # a vertex
        e = rng.integers(0, 3, m)
        w[kind == 1, e[kind == 1]] = 0.0  # a point on an edge
        if not perturb:  # lattice points: edge midpoints, the middle of the hypotenuse's neighbourhood
            w[kind == 1] = np.where(w[kind == 1] > 0, 0.5, 0.0)
            w[kind == 2] = np.array([0.5, 0.25, 0.25])
        w /= w.sum(axis=1, keepdims=True)
        tg = np.einsum("nk,nkc->nc", w, P[tri])
        if perturb:
            tg *= 1.0 + rng.choice(eps, (m, 1))
        return tg

    def unit(v):
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def aimed(m, dist, inside):
        tri = pick_tris(m)
        tg = targets(tri)
        d = unit(rng.normal(size=(m, 3)))
        ro = tg + dist * ext * d
        if inside:  # keep the origin inside the box: mirror the components that leave it
            out = (ro < lo) | (ro > hi)
            ro = np.where(out, tg - dist * ext * d, ro)
            ro = np.clip(ro, lo, hi)
        return ro, unit(tg - ro), np.where(rng.random(m) < 0.1, tri, -1)

    if family in ("aimed", "scaled"):
        ro, rd, ex = aimed(n, 0.05, True)
        if family == "scaled":
            rd = rd * np.where(np.arange(n) < n // 2, 1e-3, 1e3)[:, None]
    elif family == "far":
        ro, rd, ex = aimed(n, np.where(np.arange(n) % 2 == 0, 1e2, 1e4)[:, None], False)
    elif family == "secondary":
        src = pick_tris(n, p_coin=0.02)
        w = rng.dirichlet(np.ones(3), n)
        ro = np.einsum("nk,nkc->nc", w, P[src])
        nrm = unit(np.cross(P[src, 1] - P[src, 0], P[src, 2] - P[src, 0])) * rng.choice([-1.0, 1.0], (n, 1))
        a = unit(np.cross(nrm, unit(rng.normal(size=(n, 3)))))
        b = np.cross(nrm, a)
        u1, u2 = rng.random(n), rng.random(n)
        r, ph = np.sqrt(u1), 2 * np.pi * u2
        rd = (r * np.cos(ph))[:, None] * a + (r * np.sin(ph))[:, None] * b + np.sqrt(1 - u1)[:, None] * nrm
        shadow = rng.random(n) < 0.5
        # the nearest of four candidate targets, so that fewer of these rays end on an occluder
        cand = np.stack([targets(pick_tris(n, p_coin=0.2), eps=(0.0, 0.0, 0.0, 1e-15, -1e-15, 1e-12, -1e-12)) for _ in range(4)])
        tg = cand[np.argmin(np.linalg.norm(cand - ro, axis=2), axis=0), np.arange(n)]
        rd = np.where(shadow[:, None], unit(tg - ro), rd)
        ex = src
    elif family == "axis":
        tri = pick_tris(n, p_coin=0.1, lattice_only=True)
        tg = targets(tri, perturb=False)
        V = P[np.concatenate([lat, coin[coin < R["coincident"][0] + 32]])].reshape(-1, 3)  # lattice vertex coordinates
        other = V[rng.integers(0, len(V), n)]
        rows = np.arange(n)
        line = rng.random(n) < 0.5
        # along a lattice line, at a vertex: the origin is that vertex with one coordinate from another lattice vertex
        tg[line] = P[tri[line], rng.integers(0, 3, int(line.sum()))]
        ax = rng.integers(0, 3, n)
        ro = tg.copy()
        ro[rows[line], ax[line]] = other[rows[line], ax[line]]
        same = line & (ro[rows, ax] == tg[rows, ax])
        ro[rows[same], ax[same]] = V.min(axis=0)[ax[same]]  # the pick was the vertex's own coordinate: the lowest one
        # inside the facet's lattice plane, at a vertex, an edge midpoint or an interior point: the origin is another
        # lattice vertex moved into that plane
        plane = np.argmin(P[tri].max(axis=1) - P[tri].min(axis=1), axis=1)
        ro[~line] = other[~line]
        ro[rows[~line], plane[~line]] = P[tri[~line], 0, plane[~line]]
        d = tg - ro  # exact zeros where the coordinates are equal
        nz = np.linalg.norm(d, axis=1) > 0
        d[~nz] = (0.0, -1.0, 0.0)
        rd = unit(d)
        rd = np.where((rd == 0) & (rng.random((n, 3)) < 0.5), -0.0, rd)
        assert ((rd == 0).sum(axis=1) >= 1).all()
        ex = np.full(n, -1)
    else:
        raise ValueError(family)
    rd[-1] = np.nan
    return np.ascontiguousarray(ro), np.ascontiguousarray(rd), np.asarray(ex, np.int32)


# ---- light-prep stress: lights whose cull thresholds a shading point can sit on, at any place and size ----
# (tests/prepcases.py, tests/test_prep_stress.py, tests/test_prep_stress_cpu.py)
PREP_KINDS = ("plain", "hard", "few")
PREP_PANEL = {"plain": (14, 13), "hard": (14, 13), "few": (5, 6)}  # quads of the light panel
PREP_BLINDS, PREP_STRIPS = (-0.4, 1.2), 6
# light triangles per kind: the panel, the 16 x 8 sphere, and for "hard" the blinds and four 8 x 4 tiny spheres
PREP_NLIGHTS = {"plain": 2 * 14 * 13 + 224, "hard": 2 * 14 * 13 + 224 + len(PREP_BLINDS) * 2 * PREP_STRIPS * 2 + 4 * 48,
                "few": 2 * 5 * 6}


def prep_stress(outdir, offset=(0, 0, 0), scale=1.0, kind="plain"):
    """The floor and block under lights, written at scale * (p + offset) with every digit (offset in units of the
    scaled scene's own unit, as ray_stress's is; the scene is about 8 units wide), the XML camera moved with it.
      plain  a down-facing light panel of 14 x 13 quads, tilted 0.1 in x (no light normal is an axis; its corners at
             (+x, -z) and (-x, +z) belong to one triangle each), and a 16 x 8 sphere light low beside the block: 588
             light triangles, 10 chunks; from the floor and the block's faces chunks lie above, below and across the
             tangent plane;
      hard   plain plus two of slivers' edge-on blinds and four of tiny_far's tiny distant lights;
      few    the panel alone with 5 x 6 quads: 60 light triangles (k_prep_lane)."""
    if kind not in PREP_KINDS:
        raise ValueError(kind)
    obj, mtls, lights = _ObjExact(), [], []
    _floor(obj, mtls)
    nx, nz = PREP_PANEL[kind]
    faces = []
    n = obj.normal(gv.norm((0.1, -1.0, 0.0)))
    x0, x1, z0, z1 = -1.5, 1.5, -1.5, 1.5
    for i in range(nx):
        for k in range(nz):
            xa, xb = x0 + (x1 - x0) * i / nx, x0 + (x1 - x0) * (i + 1) / nx
            za, zb = z0 + (z1 - z0) * k / nz, z0 + (z1 - z0) * (k + 1) / nz
            a, b = obj.vert((xa, 2.5 + 0.1 * xa, za)), obj.vert((xb, 2.5 + 0.1 * xb, za))
            c, d = obj.vert((xb, 2.5 + 0.1 * xb, zb)), obj.vert((xa, 2.5 + 0.1 * xa, zb))
            faces += [((a, n), (b, n), (c, n)), ((a, n), (c, n), (d, n))]  # facing the floor
    obj.groups.append(("panel", "panel", faces))
    mtls.append(("panel", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0))
    lights.append(("panel", (2.0, 2.0, 2.0)))
    if kind != "few":
        obj.sphere("bulb", "bulb", (-1.2, 0.6, 0.5), 0.3, 16, 8)
        mtls.append(("bulb", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0))
        lights.append(("bulb", (20.0, 18.0, 15.0)))
    if kind == "hard":
        obj.groups.append(("blinds", "blinds", _blinds(obj, PREP_BLINDS, PREP_STRIPS)))
        mtls.append(("blinds", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0))
        lights.append(("blinds", (4.0, 4.0, 4.0)))
        _tiny_lights(obj, mtls, lights, (1e-2, 1e-4), ((20.0, 0.3), (45.0, 1.9)))

    def place(p):
        return tuple(scale * (x + o) for x, o in zip(p, offset))

    obj.v = [place(p) for p in obj.v]
    return _write(outdir, "prep_" + kind, obj, mtls, lights, (place(CAM[0]), place(CAM[1])))
