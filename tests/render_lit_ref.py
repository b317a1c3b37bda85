"""fp64 ray-cast reference of the renderer's shading model, flat and with the opt-in effects
(TEST INFRASTRUCTURE ONLY: the product path never imports this module).

oracle/render_ref.py pins the geometry of the images (segment ids).  This module adds the colours:
it casts the same camera rays against the same triangle model (mujoco_manip_amd/model/
render_model.json, posed by the fp64 oracle's body poses) and shades them by the model DESIGN §8
specifies, in fp64:

  flat     per face: headlight 0.3 + 0.6 max(n . z_cam, 0), directional 0.8 max(n_z, 0), point light
           0.4 max(n . dir(light - centroid), 0); the floor per pixel (checker, point light at the
           pixel's own point); the sky gradient where nothing is hit;
  shadows  a surface point loses its directional term where an opaque, non-floor triangle lies above
           it along world +z (the bins, alpha < 1, cast nothing);
  translucent bins  every front-facing bin triangle in front of the nearest opaque surface, blended
           back to front, c = 0.4 layer + 0.6 c, each layer under its own light and shadow test.

A texel-quantised shadow map may legitimately differ from a ray caster within a map texel of a
shadow's edge.  The masks name the pixels where it may not: up-rays from the surface point and from
the 8 points offset by +-d in world x and y, d = 1.5 map texels.  `certain_shadow`: all nine hit a
caster at least 10 mm above the point (and the face is turned toward the light: a face turned away has
no directional term to lose, so no mode can change its colour); `certain_lit`: none of the nine hits
anything.  Everything else is uncertain.

The flat image alone (tests/test_render_flat_pixels.py): Scene holds the posed model, the camera's rays and the
shading, stated once for render() and for Scene.flat(rows, offset), which casts only the rows asked for, through
pixel centres moved by a sub-pixel offset, with no up-rays, and also returns the face, the hit point and the
depth key's scaled inverse depth of the nearest hit and of the nearest hit on another face.  flat_certain() makes
of them the mask of pixels where a rasteriser must agree with the ray caster.
"""
from __future__ import annotations

import numpy as np
import render_ref as RR

TEXEL = 2.0 / 256.0          # the shadow map's texel (m): 256 texels over the 2 m square
MARGIN = 1.5 * TEXEL         # offset of the 8 neighbour up-rays
CERTAIN_HEIGHT = 0.010       # a certain shadow's caster lies at least this far above the point
LIGHT_POS = np.array([0.5, 0.5, 1.5])
UP_EPS = 1e-5                # an up-ray's own surface is not a hit
MAX_LAYERS = 6
_OFFS = np.array([[0, 0]] + [[dx, dy] for dx in (-1, 0, 1) for dy in (-1, 0, 1) if dx or dy], float) * MARGIN


def to_u8(c):
    """The renderer's rounding of a colour in [0, 1]: floor(255 c + 0.5)."""
    return np.floor(np.clip(c, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def world_vertices(body_pose):
    m = RR.model()
    V = np.empty_like(m["verts"])
    for b in np.unique(m["vert_body"]):
        R, p = body_pose(int(b))
        sel = m["vert_body"] == b
        V[sel] = m["verts"][sel] @ np.asarray(R).T + p
    return V


def tri_alpha():
    m = RR.model()
    return np.array([m["materials"][k].get("alpha", 1.0) for k in m["tri_mat"]], float)


class UpCaster:
    """Up-rays (world +z) against the casters: the opaque triangles that are not the floor."""

    def __init__(self, V):
        m = RR.model()
        cast = (tri_alpha() >= 1.0) & (np.array([m["materials"][k]["seg"] for k in m["tri_mat"]]) != 1)
        T = m["tris"][cast]
        self.A, self.B, self.C = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]

    def cast(self, P):
        """For points P [n, 3]: (hit anything above, height of the highest caster above or 0)."""
        n = len(P)
        any_hit = np.zeros(n, bool)
        tmax = np.zeros(n)
        if n == 0:
            return any_hit, tmax
        order = np.argsort(P[:, 0], kind="stable")
        xs = P[order, 0]
        x0 = np.minimum(np.minimum(self.A[:, 0], self.B[:, 0]), self.C[:, 0])
        x1 = np.maximum(np.maximum(self.A[:, 0], self.B[:, 0]), self.C[:, 0])
        lo, hi = np.searchsorted(xs, x0, "left"), np.searchsorted(xs, x1, "right")
        for k in np.nonzero(hi > lo)[0]:
            a, b, c = self.A[k], self.B[k], self.C[k]
            d = (b[0] - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (b[1] - a[1])
            if abs(d) < 1e-14:  # a vertical triangle: no area under the light
                continue
            idx = order[lo[k]:hi[k]]
            px, py = P[idx, 0] - a[0], P[idx, 1] - a[1]
            u = (px * (c[1] - a[1]) - (c[0] - a[0]) * py) / d
            v = ((b[0] - a[0]) * py - px * (b[1] - a[1])) / d
            t = a[2] + u * (b[2] - a[2]) + v * (c[2] - a[2]) - P[idx, 2]
            hit = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > UP_EPS)
            sel = idx[hit]
            any_hit[sel] = True
            tmax[sel] = np.maximum(tmax[sel], t[hit])
        return any_hit, tmax

    def classify(self, P):
        """(shadowed [n]: the centre up-ray hits a caster; certain_shadow; certain_lit) of points P."""
        n = len(P)
        Q = np.repeat(P[:, None, :], 9, 1)
        Q[:, :, :2] += _OFFS[None]
        hit, tmax = self.cast(Q.reshape(-1, 3))
        hit, tmax = hit.reshape(n, 9), tmax.reshape(n, 9)
        return hit[:, 0], (tmax >= CERTAIN_HEIGHT).all(1), ~hit.any(1)


# The flat model's constants, stated once: render() and Scene.flat() both shade through Scene.shade.
# A test may alter one at a time (tests/test_render_flat_pixels.py: the mutation checks).
FLAT_MODEL = {"directional": 0.8,      # the scene's directional light (dir 0 0 -1)
              "point_at": "centroid",  # where a face takes the point light: its centroid, or "vertex" (its first)
              "checker_shift": 0}      # the floor's checker, shifted by this many squares along x
# the cameras' depth ranges (znear, zfar): mujoco_manip_amd/csrc/mmx_render.hip, "depth range of the camera"
DEPTH_RANGE = {"overhead": (0.5, 2.5), "wrist": (0.01, 4.0)}
KEY_QUANTA = float(1 << 20)  # the depth key holds 20 bits of the scaled inverse depth q


class Scene:
    """The triangle model posed by body_pose, seen by camera cam_name at S x S: the camera's rays, their
    hits per image row (Moeller-Trumbore against the triangles whose screen rows the row can meet) and
    the flat shading model of a hit."""

    def __init__(self, body_pose, cam_name: str, S: int, model=None):
        m = RR.model()
        mdl = dict(FLAT_MODEL, **(model or {}))
        self.S, self.cam_name, self.mdl = S, cam_name, mdl
        self.V = V = world_vertices(body_pose)
        self.cR, self.cp = cR, cp = RR.camera_pose(cam_name, body_pose)
        fovy = [c for c in m["cameras"] if c["name"] == cam_name][0]["fovy"]
        self.f = f = (S / 2.0) / np.tan(np.radians(fovy) / 2.0)
        self.tris = tris = m["tris"]
        A, B, C = V[tris[:, 0]], V[tris[:, 1]], V[tris[:, 2]]
        self.e1, self.e2 = e1, e2 = B - A, C - A
        self.nrm = nrm = np.cross(e1, e2)
        nlen = np.linalg.norm(nrm, axis=1)
        nu = nrm / np.where(nlen > 0, nlen, 1.0)[:, None]
        cen = (A + B + C) / 3.0
        to_l = LIGHT_POS - (cen if mdl["point_at"] == "centroid" else A)
        to_l /= np.linalg.norm(to_l, axis=1)[:, None]
        self.base = 0.3 + 0.6 * np.maximum(nu @ cR[:, 2], 0.0) + 0.4 * np.maximum((nu * to_l).sum(1), 0.0)
        self.direc = mdl["directional"] * np.maximum(nu[:, 2], 0.0)
        mats = m["materials"]
        self.rgb1 = np.array([mats[k]["rgb"] for k in m["tri_mat"]], float)
        self.is_floor = m["tri_seg"] == 1
        self.floor_mat = [x for x in mats if x["seg"] == 1][0]
        self.tri_seg = m["tri_seg"]
        self.tvec_a = cp[None, :] - A
        self.qvec_a = np.cross(self.tvec_a, e1)
        self.e2q_a = np.einsum("tk,tk->t", e2, self.qvec_a)
        # image rows each triangle can meet: a triangle wholly in front of the camera projects to a screen
        # triangle, and a ray of row r (image y = r + 0.5) meets it only inside that triangle's rows
        self.vc = vc = (V - cp) @ cR
        front_v = -vc[:, 2] > 1e-3
        vrow = S / 2.0 - f * vc[:, 1] / np.where(front_v, -vc[:, 2], 1.0)
        safe = front_v[tris].all(1)
        self.rmin = np.where(safe, vrow[tris].min(1), -np.inf)
        self.rmax = np.where(safe, vrow[tris].max(1), np.inf)
        # a triangle wholly behind the camera's plane meets no row: a hit's ray parameter is its camera
        # depth, a convex combination of the vertices' depths, and hits() asks for more than 1e-6
        behind = (-vc[:, 2])[tris].max(1) <= 1e-6
        self.rmin = np.where(behind, np.inf, self.rmin)
        self.rmax = np.where(behind, -np.inf, self.rmax)

    def rays(self, r: int, offset=(0.0, 0.0)):
        """World directions [S, 3] of row r's rays (camera z = -1: a hit's ray parameter is its camera
        depth), through the pixel centres moved by offset = (dx, dy) pixels."""
        S, f = self.S, self.f
        cols = (np.arange(S) + 0.5 + offset[0] - S / 2.0) / f
        y = -(r + 0.5 + offset[1] - S / 2.0) / f
        return np.stack([cols, np.full(S, y), -np.ones(S)], 1) @ self.cR.T

    def hits(self, r: int, Dr, dy=0.0):
        """Ray parameters [S, T] of row r's rays Dr against every triangle's front face (inf = no hit)."""
        keep = np.nonzero((self.rmin - 1.0 <= r + 0.5 + dy) & (r + 0.5 + dy <= self.rmax + 1.0))[0]
        t = np.full((len(Dr), len(self.tris)), np.inf)
        if len(keep):
            e1k, e2k = self.e1[keep], self.e2[keep]
            pvec = np.cross(Dr[:, None, :], e2k[None, :, :])
            det = np.einsum("tk,stk->st", e1k, pvec)
            inv = 1.0 / np.where(np.abs(det) < 1e-18, np.inf, det)
            u = np.einsum("tk,stk->st", self.tvec_a[keep], pvec) * inv
            v = np.einsum("sk,tk->st", Dr, self.qvec_a[keep]) * inv
            tk = self.e2q_a[keep][None, :] * inv
            front = np.einsum("sk,tk->st", Dr, self.nrm[keep]) < 0
            hit = front & (u >= 0) & (v >= 0) & (u + v <= 1) & (tk > 1e-6)
            t[:, keep] = np.where(hit, tk, np.inf)
        return t

    def shade(self, k, t, D, dark=None):
        """Colours [..., 3] of surface k [...] (triangle ids, -1 = none: the sky) hit at ray parameter t on
        rays D [..., 3]; dark [...]: where the directional term is lost (None: nowhere, the flat image).
        Also the hit points [..., 3] and the floor's checker parity [...] (False off the floor)."""
        cR, cp = self.cR, self.cp
        P = cp + D * np.where(np.isfinite(t), t, 0.0)[..., None]
        valid = k >= 0
        kk = np.where(valid, k, 0)
        fl = self.is_floor[kk] & valid
        # the floor: the point light at the pixel's own point, the checker
        dl = LIGHT_POS - P
        point_floor = 0.4 * LIGHT_POS[2] / np.linalg.norm(dl, axis=-1)
        b_light = np.where(fl, 0.3 + 0.6 * max(cR[2, 2], 0.0) + point_floor, self.base[kk])
        d_light = np.where(fl, self.mdl["directional"], self.direc[kk])
        light = b_light + (d_light if dark is None else np.where(dark, 0.0, d_light))
        light = np.minimum(light, 3.99)
        fm = self.floor_mat
        sq = fm["checker"]
        alt = ((np.floor(P[..., 0] / sq + self.mdl["checker_shift"]) + np.floor(P[..., 1] / sq)).astype(int) & 1).astype(bool)
        colour = np.where(fl[..., None], np.where(alt[..., None], np.array(fm["rgb2"]), np.array(fm["rgb"])), self.rgb1[kk])
        out = np.minimum(colour * light[..., None], 1.0)
        sky = 0.5 * (D[..., 2] / np.linalg.norm(D, axis=-1) + 1.0)
        out = np.where(valid[..., None], out, sky[..., None] * np.array([0.3, 0.5, 0.7]))
        return out, P, alt & fl

    def flat(self, rows=None, offset=(0.0, 0.0)):
        """The flat image on the given image rows (all by default), rays through the pixel centres moved by
        offset = (dx, dy) pixels; no shadow up-rays.  A dict of [n, S(, 3)] arrays: rows [n]; k (the face hit,
        -1 = sky); f_flat, rgb_flat, seg as render() gives them; point (the hit point); floor, alt (a floor
        pixel, its checker parity); depth (camera depth of the hit, inf = none), q = (1 / depth - 1 / zfar) /
        (1 / znear - 1 / zfar), the depth key's scaled inverse depth; depth2, q2: the same of the nearest
        hit on a different face (q2 = -inf where there is none)."""
        S = self.S
        rows = np.arange(S) if rows is None else np.asarray(rows, int)
        n, ar = len(rows), np.arange(S)
        k = np.full((n, S), -1)
        t1, t2 = np.full((n, S), np.inf), np.full((n, S), np.inf)
        D = np.empty((n, S, 3))
        for i, r in enumerate(rows):
            D[i] = self.rays(int(r), offset)
            t = self.hits(int(r), D[i], offset[1])
            j = np.argmin(t, 1)
            t1[i] = t[ar, j]
            k[i] = np.where(np.isfinite(t1[i]), j, -1)
            t[ar, j] = np.inf
            t2[i] = t.min(1)
        f_flat, P, alt = self.shade(k, t1, D)
        zn, zf = DEPTH_RANGE[self.cam_name]

        def q_of(t):
            return np.where(np.isfinite(t), (1.0 / np.where(np.isfinite(t), t, 1.0) - 1.0 / zf) / (1.0 / zn - 1.0 / zf), -np.inf)

        kk = np.where(k >= 0, k, 0)
        return {"rows": rows, "k": k, "f_flat": f_flat, "rgb_flat": to_u8(f_flat),
                "seg": np.where(k >= 0, self.tri_seg[kk], 0).astype(np.uint8), "point": P,
                "floor": self.is_floor[kk] & (k >= 0), "alt": alt, "depth": t1, "q": q_of(t1), "depth2": t2, "q2": q_of(t2)}

    def screen(self):
        """Per vertex: screen x, y (pixels, row 0 at the top) and camera depth, in fp64 (what rend_project
        computes in fp32); a vertex at or behind the camera's plane gets nan coordinates."""
        d = -self.vc[:, 2]
        ok = d > 0
        iz = 1.0 / np.where(ok, d, np.nan)
        return self.S / 2.0 + self.f * self.vc[:, 0] * iz, self.S / 2.0 - self.f * self.vc[:, 1] * iz, d


SUBPIXEL = 1.0 / 16.0  # the certainty mask's sub-pixel offset (pixels)
TIE_QUANTA = 16        # ... and its depth separation, in depth-key quanta


def flat_certain(scene: Scene, rows=None):
    """The flat image of scene.flat(rows) with the mask of pixels where a rasteriser sampling the same
    pixel centres in fp32 must show the ray caster's face.  Conditions, not tolerances:
      stable    the rays through the centre and through the four points (+-1/16, +-1/16) px off it hit the
                same face (the floor's triangles count as one face: the plane) and, on the floor, the same
                checker colour; fp32 poses and projection move a vertex by ~1e-3 px at 224 px
                (tests/test_render_flat_pixels.py asserts < 1/64 px on the fixture);
      no_tie    the nearest different face along the centre ray lies at least 16 depth-key quanta
                (16 / 2^20 in q) behind; a floor or sky pixel has no other face on its ray at all: the kernel
                does not rasterise the floor, it shows it (or the sky) where no triangle covers the pixel;
      in_range  the hit's camera depth lies in [znear, zfar] and no vertex of the face is nearer than znear
                (the kernel drops such a face whole: DESIGN §8).  The floor, intersected per pixel, has
                neither limit in the kernel; only its depth range is asked for here.
    Adds stable, no_tie, in_range and certain (all three) to the dict."""
    c = scene.flat(rows)
    face = np.where(c["floor"], -2, c["k"])
    stable = np.ones(face.shape, bool)
    for dx in (-SUBPIXEL, SUBPIXEL):
        for dy in (-SUBPIXEL, SUBPIXEL):
            o = scene.flat(rows, (dx, dy))
            stable &= (np.where(o["floor"], -2, o["k"]) == face) & (o["alt"] == c["alt"])
    hit = c["k"] >= 0
    raster = hit & ~c["floor"]
    gap = np.where(raster, c["q"], 0.0) - np.where(raster, c["q2"], -np.inf)
    no_tie = np.where(raster, gap >= TIE_QUANTA / KEY_QUANTA, ~np.isfinite(c["depth2"]))
    zn, zf = DEPTH_RANGE[scene.cam_name]
    vdepth = -scene.vc[:, 2]
    face_near = vdepth[scene.tris].min(1)[np.where(hit, c["k"], 0)]
    in_range = ~hit | ((c["depth"] >= zn) & (c["depth"] <= zf) & (c["floor"] | (face_near >= zn)))
    c.update(stable=stable, no_tie=no_tie, in_range=in_range, certain=stable & no_tie & in_range)
    return c


def render(body_pose, cam_name: str, S: int):
    """The reference images of camera `cam_name` at S x S.  Returns a dict of [S, S(, 3)] arrays:
    rgb_flat, rgb_shadows, rgb_translucent, rgb_lit (both effects) as uint8; the same as floats in
    [0, 1] under f_flat, ...; seg (uint8, nearest surface with the bins counted); layers (translucent
    layers in front of the nearest opaque surface); certain_shadow / certain_lit (of the nearest
    surface with the bins counted: what the shadows-only mode shades); certain_lit_all (every point the
    lit mode shades at the pixel, the opaque surface and each layer, is certainly lit);
    translucent (layers > 0); shadowed (the reference's own verdict at the nearest surface)."""
    m = RR.model()
    sc = Scene(body_pose, cam_name, S)
    V, cp, direc = sc.V, sc.cp, sc.direc
    alpha = tri_alpha()
    is_bin = alpha < 1.0
    opaque_ids, bin_ids = np.nonzero(~is_bin)[0], np.nonzero(is_bin)[0]

    # primary rays: per pixel the nearest hit overall, the nearest opaque hit, the bin hits in front of it
    k_all = np.full((S, S), -1)
    t_all = np.full((S, S), np.inf)
    k_op = np.full((S, S), -1)
    t_op = np.full((S, S), np.inf)
    lay_k = np.full((S, S, MAX_LAYERS), -1)
    lay_t = np.full((S, S, MAX_LAYERS), np.inf)
    layers = np.zeros((S, S), int)
    D = np.empty((S, S, 3))
    for r in range(S):
        D[r] = sc.rays(r)
        t = sc.hits(r, D[r])
        ar = np.arange(S)
        k = np.argmin(t, 1)
        t_all[r] = t[ar, k]
        k_all[r] = np.where(np.isfinite(t_all[r]), k, -1)
        to = t[:, opaque_ids]
        k = np.argmin(to, 1)
        t_op[r] = to[ar, k]
        k_op[r] = np.where(np.isfinite(t_op[r]), opaque_ids[k], -1)
        tb = np.where(t[:, bin_ids] < t_op[r][:, None], t[:, bin_ids], np.inf)
        layers[r] = np.isfinite(tb).sum(1)
        o = np.argsort(tb, 1, kind="stable")[:, :MAX_LAYERS]
        lay_t[r] = np.take_along_axis(tb, o, 1)
        lay_k[r] = np.where(np.isfinite(lay_t[r]), bin_ids[o], -1)
    assert layers.max() <= MAX_LAYERS, "more translucent layers than the reference keeps"

    up = UpCaster(V)
    classified = {}

    def shade(k, t, shadow_mode):
        """Colours [S, S, 3] of surface k (triangle ids, -1 = none) hit at ray parameter t, with or
        without the shadow test; also the shadow classification of the points."""
        P = cp[None, None, :] + D * np.where(np.isfinite(t), t, 0.0)[..., None]
        valid = k >= 0
        kk = np.where(valid, k, 0)
        if id(k) not in classified:  # the up-rays of a surface do not depend on the mode
            sh = np.zeros((S, S), bool)
            cs = np.zeros((S, S), bool)
            cl = np.ones((S, S), bool)
            sh[valid], cs[valid], cl[valid] = up.classify(P[valid])
            classified[id(k)] = (k, sh, cs, cl)
        _, sh, cs, cl = classified[id(k)]
        cs = cs.copy()
        faces_light = direc[kk] > 0.0
        cs &= faces_light & valid
        out = sc.shade(k, t, D, shadow_mode & sh)[0]
        return out, sh & valid, cs, cl

    lay_ks = [np.ascontiguousarray(lay_k[..., j]) for j in range(MAX_LAYERS)]
    res = {}
    flat, sh_all, cs_all, cl_all = shade(k_all, t_all, False)
    res["f_flat"] = flat
    res["f_shadows"] = shade(k_all, t_all, True)[0]
    res["shadowed"], res["certain_shadow"], res["certain_lit"] = sh_all, cs_all, cl_all
    cl_every = None
    for mode, name in ((False, "f_translucent"), (True, "f_lit")):
        c, _, _, cl_every = shade(k_op, t_op, mode)
        for j in range(MAX_LAYERS - 1, -1, -1):  # back to front
            has = lay_k[..., j] >= 0
            if not has.any():
                continue
            lc, _, _, cl_j = shade(lay_ks[j], lay_t[..., j], mode)
            c = np.where(has[..., None], 0.4 * lc + 0.6 * c, c)
            cl_every = cl_every & cl_j
        res[name] = c
    res["certain_lit_all"] = cl_every & cl_all
    for name in ("flat", "shadows", "translucent", "lit"):
        res["rgb_" + name] = to_u8(res["f_" + name])
    res["seg"] = np.where(k_all >= 0, m["tri_seg"][np.where(k_all >= 0, k_all, 0)], 0).astype(np.uint8)
    res["layers"] = layers
    res["translucent"] = layers > 0
    res["k_all"], res["k_opaque"], res["t_all"] = k_all, k_op, t_all
    return res


def interior(mask):
    """One-pixel image-space erosion (4-neighbourhood): the pixels whose neighbours are in the mask too."""
    m = np.asarray(mask, bool)
    p = np.pad(m, 1)
    return m & p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
