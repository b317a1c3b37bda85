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


def render(body_pose, cam_name: str, S: int):
    """The reference images of camera `cam_name` at S x S.  Returns a dict of [S, S(, 3)] arrays:
    rgb_flat, rgb_shadows, rgb_translucent, rgb_lit (both effects) as uint8; the same as floats in
    [0, 1] under f_flat, ...; seg (uint8, nearest surface with the bins counted); layers (translucent
    layers in front of the nearest opaque surface); certain_shadow / certain_lit (of the nearest
    surface with the bins counted: what the shadows-only mode shades); certain_lit_all (every point the
    lit mode shades at the pixel, the opaque surface and each layer, is certainly lit);
    translucent (layers > 0); shadowed (the reference's own verdict at the nearest surface)."""
    m = RR.model()
    V = world_vertices(body_pose)
    cR, cp = RR.camera_pose(cam_name, body_pose)
    fovy = [c for c in m["cameras"] if c["name"] == cam_name][0]["fovy"]
    f = (S / 2.0) / np.tan(np.radians(fovy) / 2.0)
    tris = m["tris"]
    A, B, C = V[tris[:, 0]], V[tris[:, 1]], V[tris[:, 2]]
    e1, e2 = B - A, C - A
    nrm = np.cross(e1, e2)
    nlen = np.linalg.norm(nrm, axis=1)
    nu = nrm / np.where(nlen > 0, nlen, 1.0)[:, None]
    cen = (A + B + C) / 3.0
    to_l = LIGHT_POS - cen
    to_l /= np.linalg.norm(to_l, axis=1)[:, None]
    base = 0.3 + 0.6 * np.maximum(nu @ cR[:, 2], 0.0) + 0.4 * np.maximum((nu * to_l).sum(1), 0.0)
    direc = 0.8 * np.maximum(nu[:, 2], 0.0)
    mats = m["materials"]
    rgb1 = np.array([mats[k]["rgb"] for k in m["tri_mat"]], float)
    alpha = tri_alpha()
    is_bin = alpha < 1.0
    is_floor = m["tri_seg"] == 1
    floor_mat = [x for x in mats if x["seg"] == 1][0]
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
    cols = (np.arange(S) + 0.5 - S / 2.0) / f
    tvec_a = cp[None, :] - A
    qvec_a = np.cross(tvec_a, e1)
    e2q_a = np.einsum("tk,tk->t", e2, qvec_a)
    # image rows each triangle can meet: a triangle wholly in front of the camera projects to a screen
    # triangle, and a ray of row r (image y = r + 0.5) meets it only inside that triangle's rows
    vc = (V - cp) @ cR
    front_v = -vc[:, 2] > 1e-3
    vrow = S / 2.0 - f * vc[:, 1] / np.where(front_v, -vc[:, 2], 1.0)
    safe = front_v[tris].all(1)
    rmin = np.where(safe, vrow[tris].min(1), -np.inf)
    rmax = np.where(safe, vrow[tris].max(1), np.inf)
    for r in range(S):
        y = -(r + 0.5 - S / 2.0) / f
        Dr = np.stack([cols, np.full(S, y), -np.ones(S)], 1) @ cR.T
        D[r] = Dr
        keep = np.nonzero((rmin - 1.0 <= r + 0.5) & (r + 0.5 <= rmax + 1.0))[0]
        t = np.full((S, len(tris)), np.inf)
        if len(keep):
            e1k, e2k = e1[keep], e2[keep]
            pvec = np.cross(Dr[:, None, :], e2k[None, :, :])
            det = np.einsum("tk,stk->st", e1k, pvec)
            inv = 1.0 / np.where(np.abs(det) < 1e-18, np.inf, det)
            u = np.einsum("tk,stk->st", tvec_a[keep], pvec) * inv
            v = np.einsum("sk,tk->st", Dr, qvec_a[keep]) * inv
            tk = e2q_a[keep][None, :] * inv
            front = np.einsum("sk,tk->st", Dr, nrm[keep]) < 0
            hit = front & (u >= 0) & (v >= 0) & (u + v <= 1) & (tk > 1e-6)
            t[:, keep] = np.where(hit, tk, np.inf)
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
        fl = is_floor[kk] & valid
        # the floor: the point light at the pixel's own point, the checker
        dl = LIGHT_POS[None, None, :] - P
        point_floor = 0.4 * LIGHT_POS[2] / np.linalg.norm(dl, axis=2)
        b_light = np.where(fl, 0.3 + 0.6 * max(cR[2, 2], 0.0) + point_floor, base[kk])
        d_light = np.where(fl, 0.8, direc[kk])
        light = b_light + np.where(shadow_mode & sh, 0.0, d_light)
        light = np.minimum(light, 3.99)
        sq = floor_mat["checker"]
        alt = ((np.floor(P[..., 0] / sq) + np.floor(P[..., 1] / sq)).astype(int) & 1).astype(bool)
        colour = np.where(fl[..., None], np.where(alt[..., None], np.array(floor_mat["rgb2"]), np.array(floor_mat["rgb"])),
                          rgb1[kk])
        out = np.minimum(colour * light[..., None], 1.0)
        sky = 0.5 * (D[..., 2] / np.linalg.norm(D, axis=2) + 1.0)
        out = np.where(valid[..., None], out, sky[..., None] * np.array([0.3, 0.5, 0.7]))
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
