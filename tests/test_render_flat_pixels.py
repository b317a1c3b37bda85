"""The flat camera image (mmx_render_kernel) pinned per pixel against the fp64 ray caster, at the
image sizes where the kernel's raster layout changes shape.

States: tests/golden/render_states.npz (made by tests/golden/make_render_states.py with the fp64 oracle): the
keyframe, the keyframe with the arm turned away, and five phases of two expert episodes (red cube -> red bin,
blue cube -> green bin).  Reference: tests/render_lit_ref.py, Scene.flat on the rows asked for, the same
shading code test_render_lit.py's reference uses.

The mask (render_lit_ref.flat_certain) is a set of conditions, not a tolerance: the rays through a pixel's centre
and through the four points (+-1/16, +-1/16) px off it hit the same face (on the floor: the same checker colour);
the nearest other face on the centre ray is at least 16 depth-key quanta behind; the hit lies inside the camera's
depth range and its face has no vertex nearer than znear (the kernel drops such a face whole: a documented limit,
DESIGN §8, that these tests leave as it is).  On every pixel of the mask, with no share and no exception:

  the segment id is the reference's;
  |u8 - 255 f_flat| <= 0.5 + 255 * 2^-13 per channel (about 0.531), against the reference's float colour: the
  kernel rounds floor(255 c + 0.5) (0.5) and cuts a face's light down to steps of 2^-14 (mmx_render.hip, "the
  face's packed colour"; material colours are at most 1, so at most 255 * 2^-14), and a second 2^-14 covers the
  fp32 rounding of the normal, the light sum and the floor term's rsqrtf.

Sizes (Sg = the size rounded up to 16; band rows by rend_band_rows; two bands per workgroup), asserted through
mmx_render_band_rows / mmx_render_bands_per_workgroup so that a retuned MMR_BAND_PX names the sizes that lost
their purpose:

  size  Sg   band rows  bands  workgroups
   16    16     16        1       1        a single tile
   20    32     32        1       1        partial tiles, byte stores, tiles outside the image, background-table
                                           stride Sg != size
  128   128     64        2       1        the second band through the reused z-buffer
  150   160     40        4       2        a band height that is no multiple of 16, the last band cut by the image
                                           edge, byte stores in an image of several workgroups
  224   224     32        7       4        the default size; the last workgroup has one band

At 16 and 20 px every state and row; at 128, 150 and 224 px the turned keyframe and the held cube, on the rows
within 2 of a band boundary or of the image's top and bottom edge and every 8th row besides.

CPU: the premises (the mask's floors, the band table, certain pixels and straddling faces at every band boundary,
the large and the tiny raster path, every material), the fp32 projection against the mask's 1/16 px, the new
reference path against render(), and mutation checks: five single errors put into the reference's model each break
the bound on certain pixels.

Measured (profiles/r17_render_flat_margins.json).  CPU: the fp32 restatement of the projection moves no vertex
within an image side of a 224 px image by more than 0.00064 px (wrist; overhead 0.00003; the mask's offset / 4 is
0.0156 px); the mask keeps 0.68 - 0.95 of an image at 16 and 20 px and 0.94 - 0.98 at 128 px and up; the depth-range
condition excludes no pixel of any case; each single error breaks the bound on 0.86 - 0.99 of the certain pixels
of its clearest case; all references of the module take 4 s (pytest --durations: the premises test, which
computes them, 4.1 s; every other CPU test under 1 s).  MI355X: every one of the 78,426 certain pixels has the
reference's segment id and lies inside the bound; worst |u8 - 255 f| per size, overhead / wrist: 16 px 0.4993 /
0.5000, 20 px 0.4975 / 0.5057, 128 px 0.5000 / 0.5000, 150 px 0.4999 / 0.5000, 224 px 0.5000 / 0.5002 (bound
0.5311); each GPU test under 0.3 s beside the references.
"""
import os

import numpy as np
import pytest

try:  # before the library is loaded, as in a run of the whole suite (test_render.py imports it when collected):
    import torch  # noqa: F401  the CPU tests below load libmmx.so, and the HIP runtime must be torch's
except ImportError:
    pass

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMS = ("overhead", "wrist")
SMALL, BIG = (16, 20), (128, 150, 224)
# size -> (Sg, band rows, bands, workgroups)
BAND_TABLE = {16: (16, 16, 1, 1), 20: (32, 32, 1, 1), 128: (128, 64, 2, 1), 150: (160, 40, 4, 2), 224: (224, 32, 7, 4)}
BOUND = 0.5 + 255.0 * 2.0 ** -13
SMALL_AREA, TINY_AREA = 2048, 64  # MMR_SMALL_AREA, MMR_TINY (mmx_render.hip): box areas that choose the raster path
SEG_NAMES = {2: "table", 6: "red cube", 7: "green cube", 8: "blue cube", 9: "robot"}
SEG_BINS = (3, 4, 5)


# ------------------------------------------------------------------------------------------ cases
_FIX = {}


def _fixture():
    if not _FIX:
        z = np.load(os.path.join(REPO, "tests", "golden", "render_states.npz"))
        _FIX.update(qpos=z["qpos"], labels=[str(x) for x in z["labels"]])
    return _FIX


def _state_ids(size):
    lab = _fixture()["labels"]
    return list(range(len(lab))) if size in SMALL else [lab.index("keyframe_turned"), lab.index("held")]


def _layout(size):
    """(band rows, bands, workgroups) of an image size, from the library."""
    from mujoco_manip_amd import _lib

    L = _lib.load()
    rows, bpw = L.mmx_render_band_rows(size), L.mmx_render_bands_per_workgroup()
    bands = -(-size // rows)
    return rows, bands, -(-bands // bpw)


def _boundaries(size):
    rows = _layout(size)[0]
    return list(range(rows, size, rows))


def _rows(size):
    if size in SMALL:
        return np.arange(size)
    edges = [0, size] + _boundaries(size)
    return np.array([r for r in range(size) if r % 8 == 0 or any(e - 2 <= r < e + 2 for e in edges)])


_POSE, _SCENE, _REF = {}, {}, {}


def _pose(i):
    if i not in _POSE:
        import oracle_py as O

        e = O.OracleEnv()
        e.set_state(qpos=_fixture()["qpos"][i].astype(float))
        e.mj_forward()
        cache = {}

        def pose(b):
            if b not in cache:
                p, R = e.body(b)
                cache[b] = (R, p)
            return cache[b]

        _POSE[i] = pose
    return _POSE[i]


def _scene(i, cam, size):
    import render_lit_ref as LR

    if (i, cam, size) not in _SCENE:
        _SCENE[i, cam, size] = LR.Scene(_pose(i), cam, size)
    return _SCENE[i, cam, size]


def _ref(i, cam, size):
    """The reference's flat image and certainty mask of state i, computed once per (state, camera, size)."""
    import render_lit_ref as LR

    if (i, cam, size) not in _REF:
        _REF[i, cam, size] = LR.flat_certain(_scene(i, cam, size), _rows(size))
    return _REF[i, cam, size]


def _cases(sizes=SMALL + BIG):
    return [(size, i, cam) for size in sizes for i in _state_ids(size) for cam in CAMS]


def _boxes(i, cam, size):
    """Per triangle the kernel's pixel box before band clipping (bx0, bx1, by0, by1; inclusive) from the fp64
    screen vertices, and whether the kernel rasterises the face: not the floor, no vertex nearer than znear,
    front-facing (negative screen area)."""
    import render_lit_ref as LR

    sc = _scene(i, cam, size)
    sx, sy, d = sc.screen()
    t = sc.tris
    ok = (d[t] >= LR.DEPTH_RANGE[cam][0]).all(1) & ~sc.is_floor
    x, y = np.where(ok[:, None], sx[t], 0.0), np.where(ok[:, None], sy[t], 0.0)
    area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
    ok &= area < -1e-12
    bx0 = np.maximum(0, np.ceil(x.min(1) - 0.5)).astype(int)
    bx1 = np.minimum(size - 1, np.floor(x.max(1) - 0.5)).astype(int)
    by0 = np.maximum(0, np.ceil(y.min(1) - 0.5)).astype(int)
    by1 = np.minimum(size - 1, np.floor(y.max(1) - 0.5)).astype(int)
    return bx0, bx1, by0, by1, ok & (bx0 <= bx1) & (by0 <= by1)


def _violations(u8, ref):
    """Per pixel: a channel of u8 farther than BOUND from 255 f_flat."""
    return (np.abs(u8.astype(float) - 255.0 * ref["f_flat"]) > BOUND).any(-1)


# ------------------------------------------------------------------------------------------ CPU
def test_fixture_states():
    """The committed states: seven of them, float32 [n, 30], the labels make_render_states.py names, cubes of two
    colours off the table in the held and lower-to-bin states (the blue one) and the red one moved into its bin."""
    fx = _fixture()
    q = fx["qpos"]
    assert q.dtype == np.float32 and q.shape == (7, 30) and np.isfinite(q).all()
    assert fx["labels"] == ["keyframe", "keyframe_turned", "pre_grasp", "close_gripper", "held", "lower_to_bin", "retreat"]
    key = q[0]
    assert np.array_equal(q[1][1:], key[1:]) and abs(q[1][0] + 1.5708) < 1e-6
    held, retreat = q[fx["labels"].index("held")], q[fx["labels"].index("retreat")]
    assert held[25] > key[25] + 0.1 and abs(held[11] - key[11]) < 0.005  # the blue cube is up, the red one is not
    assert np.linalg.norm(retreat[9:11] - key[9:11]) > 0.1              # the red cube has been carried away


def test_band_table_through_the_exports():
    """The sizes' purposes hold for the library as built: Sg, band rows, bands and workgroups per image."""
    from mujoco_manip_amd import _lib

    L = _lib.load()
    assert L.mmx_render_bands_per_workgroup() == 2
    for size, (sg, rows, bands, wgs) in BAND_TABLE.items():
        assert (size + 15) // 16 * 16 == sg
        assert _layout(size) == (rows, bands, wgs), (size, _layout(size))
    assert BAND_TABLE[150][1] % 16 != 0 and 150 % BAND_TABLE[150][1] != 0  # a partial last tile row, a cut last band
    assert BAND_TABLE[224][2] % 2 == 1                                      # the last workgroup has one band
    assert L.mmx_render_band_rows(0) == 0 and L.mmx_render_band_rows(1025) == 0
    for size in BIG:
        r = _rows(size)
        for b in _boundaries(size):
            assert {b - 2, b - 1, b, b + 1} <= set(r.tolist())
        assert {0, 1, size - 2, size - 1} <= set(r.tolist())
        assert set(range(0, size, 8)) <= set(r.tolist()) and len(r) <= size // 8 + 4 * (len(_boundaries(size)) + 1)


def test_fp32_projection_stays_inside_the_mask_offset(margin):
    """The mask's premise: a rasteriser that samples the ray caster's pixel centres differs from it by the fp32
    rounding of poses and projection only.  A numpy float32 restatement of the kernel's vertex pass (pose the vertex,
    to camera space, rend_project) on every fixture state at 224 px, against fp64: below (1/16) / 4 px for every
    vertex at or beyond znear that lands within one image side of the image (what lies farther out reaches the
    image only through edges whose error shrinks in proportion)."""
    import render_lit_ref as LR
    import render_ref as RR

    S, m, f32 = 224, RR.model(), np.float32
    worst = {}
    for cam in CAMS:
        worst[cam] = 0.0
        for i in range(len(_fixture()["labels"])):
            sc = _scene(i, cam, S)
            sx, sy, d = sc.screen()
            W = np.empty(m["verts"].shape, f32)
            for b in np.unique(m["vert_body"]):
                R, p = _pose(i)(int(b))
                sel = m["vert_body"] == b
                W[sel] = p.astype(f32) + m["verts"][sel].astype(f32) @ np.asarray(R).astype(f32).T
            cv = (W - sc.cp.astype(f32)) @ sc.cR.astype(f32)
            fovy = [c for c in m["cameras"] if c["name"] == cam][0]["fovy"]
            half = f32(0.5) * f32(S)
            f = half / np.tan(f32(fovy) * f32(3.14159265358979 / 360.0), dtype=f32)
            iz = f32(1.0) / -cv[:, 2]
            gx, gy = half + f * cv[:, 0] * iz, half - f * cv[:, 1] * iz
            assert gx.dtype == f32 and gy.dtype == f32
            sel = (d >= LR.DEPTH_RANGE[cam][0]) & (sx > -S) & (sx < 2 * S) & (sy > -S) & (sy < 2 * S)
            assert sel.sum() > 100
            worst[cam] = max(worst[cam], float(np.abs(gx[sel] - sx[sel]).max()), float(np.abs(gy[sel] - sy[sel]).max()))
        margin(f"fp32 projection error px, 224 px, {cam}", worst[cam], LR.SUBPIXEL / 4)
    print("fp32 projection error (px) at 224 px:", worst)
    assert max(worst.values()) < LR.SUBPIXEL / 4


def test_mask_premises(margin):
    """On the fixture and the reference alone: the mask keeps enough of every image, the depth-range condition
    excludes nothing, every band boundary has, per camera and in one of the size's two states, certain pixels in
    each of the two rows on either side and a seen rasterised face whose box straddles it, the held cube's wrist image
    reaches the large and the tiny raster path, and every material owns certain pixels somewhere."""
    owners, alt_seen, sky, straddled, edge_rows = set(), set(), 0, {}, {}
    for size, i, cam in _cases():
        r = _ref(i, cam, size)
        c = r["certain"]
        share = float(c.mean())
        print(f"size {size} state {_fixture()['labels'][i]} {cam}: certain {share:.3f} stable {r['stable'].mean():.3f} "
              f"no_tie {r['no_tie'].mean():.3f}")
        margin(f"certain share {size} {_fixture()['labels'][i]} {cam}", share)
        assert share >= (0.5 if size <= 20 else 0.8), (size, i, cam, share)
        assert r["in_range"].all(), (size, i, cam, int((~r["in_range"]).sum()))
        owners |= set(np.unique(r["seg"][c & (r["k"] >= 0)]).tolist())
        alt_seen |= set(np.unique(r["alt"][c & r["floor"]]).tolist())
        sky += int((c & (r["k"] < 0)).sum())
        if size in BIG:
            rows = r["rows"].tolist()
            bx0, bx1, by0, by1, ok = _boxes(i, cam, size)
            owned = np.zeros(len(ok), bool)
            owned[np.unique(r["k"][c & (r["k"] >= 0)])] = True
            for b in _boundaries(size):
                for row in (b - 2, b - 1, b, b + 1):
                    edge_rows[size, cam, row] = edge_rows.get((size, cam, row), 0) + int(c[rows.index(row)].sum())
                # a face whose box holds rows on both sides of the boundary (queued for both bands, set up again
                # for the second) and that is seen (owns a certain pixel): in one of the size's two states
                strad = ok & (by0 < b) & (by1 >= b)
                straddled[size, cam, b] = straddled.get((size, cam, b), 0) + int((strad & owned).sum())
            if cam == "wrist" and _fixture()["labels"][i] == "held":
                band = _layout(size)[0]
                big = tiny = False
                for r0 in range(0, size, band):
                    cy0, cy1 = np.maximum(by0, r0), np.minimum(by1, min(size, r0 + band) - 1)
                    area = np.where(ok & (cy0 <= cy1), (bx1 - bx0 + 1) * (cy1 - cy0 + 1), 0)
                    inband = np.zeros(len(ok), bool)
                    rsel = (r["rows"] >= r0) & (r["rows"] < r0 + band)
                    inband[np.unique(r["k"][rsel][c[rsel] & (r["k"][rsel] >= 0)])] = True
                    big |= bool(((area > SMALL_AREA) & inband).any())
                    tiny |= bool(((area > 0) & (area <= TINY_AREA) & inband).any())
                assert big and tiny, (size, big, tiny)
    # (one state alone does not do: with the arm turned by a right angle the wrist camera's row 79 at 150 px runs
    # along a checker line of the floor, y = -0.5 m, and no pixel of it keeps its colour under the offsets)
    nb = sum(BAND_TABLE[s][2] - 1 for s in BIG)
    assert len(edge_rows) == 8 * nb and min(edge_rows.values()) >= 1, {k: v for k, v in edge_rows.items() if v < 1}
    assert len(straddled) == 2 * nb and min(straddled.values()) >= 1, straddled
    assert set(SEG_NAMES) <= owners, owners
    assert owners & set(SEG_BINS) and 1 in owners
    assert alt_seen == {False, True}
    assert sky > 0


def test_flat_path_is_the_lit_reference_flat_image():
    """Scene.flat gives render()'s rgb_flat, f_flat and seg, bit for bit, at 64 px on the keyframe; a row subset
    gives those rows; an offset of zero is the centre."""
    import render_lit_ref as LR

    i = _fixture()["labels"].index("keyframe")
    for cam in CAMS:
        full = LR.render(_pose(i), cam, 64)
        flat = LR.Scene(_pose(i), cam, 64).flat()
        for name in ("rgb_flat", "f_flat", "seg"):
            np.testing.assert_array_equal(flat[name], full[name], err_msg=f"{cam} {name}")
        np.testing.assert_array_equal(flat["k"], full["k_all"])
        np.testing.assert_array_equal(flat["depth"], full["t_all"])
        rows = [0, 5, 31, 63]
        part = LR.Scene(_pose(i), cam, 64).flat(rows, (0.0, 0.0))
        for name in ("rgb_flat", "f_flat", "seg", "q", "q2"):
            np.testing.assert_array_equal(part[name], flat[name][rows])
        hit = flat["k"] >= 0
        assert (flat["q2"][hit] <= flat["q"][hit]).all() and (flat["q"][~hit] == -np.inf).all()
        # an offset moves the image: a whole pixel to the right is the neighbouring column's ray
        moved = LR.Scene(_pose(i), cam, 64).flat(rows, (1.0, 0.0))
        np.testing.assert_array_equal(moved["k"][:, :-1], flat["k"][rows][:, 1:])


MUTATIONS = ("directional 0.8 -> 0.7", "point light at a vertex", "checker shifted by one square", "truncation",
             "red and blue swapped")


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_bound_catches_a_single_error_in_the_model(mutation, margin):
    """The reference's flat model altered one way, rounded the kernel's way, is what a kernel with that error would
    write: it must break the bound on certain pixels in at least one case.  Unaltered, it breaks it nowhere."""
    import render_lit_ref as LR

    model = {"directional 0.8 -> 0.7": {"directional": 0.7}, "point light at a vertex": {"point_at": "vertex"},
             "checker shifted by one square": {"checker_shift": 1}}.get(mutation)
    worst, where = 0.0, None
    for size, i, cam in _cases(SMALL + (128,)):
        ref = _ref(i, cam, size)
        f = LR.Scene(_pose(i), cam, size, model).flat(ref["rows"])["f_flat"] if model else ref["f_flat"]
        u8 = np.floor(np.clip(f, 0.0, 1.0) * 255.0).astype(np.uint8) if mutation == "truncation" else LR.to_u8(f)
        if mutation == "red and blue swapped":
            u8 = u8[..., ::-1]
        assert not _violations(LR.to_u8(ref["f_flat"]), ref).any()
        share = float(_violations(u8, ref)[ref["certain"]].mean())
        if share > worst:
            worst, where = share, (size, _fixture()["labels"][i], cam)
    print(f"{mutation}: breaks the bound on {worst:.4f} of the certain pixels of {where}")
    margin(f"share of certain pixels outside the bound: {mutation}", worst, case=str(where))
    assert worst > 0.0


# ------------------------------------------------------------------------------------------ GPU
def _need_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


_IMAGES = {}


def _render(size, flags=None):
    """(rgb [n, 2, S, S, 3], seg [n, 2, S, S]) of the size's states; flags None: the setter never called."""
    if (size, flags) not in _IMAGES:
        torch = _need_gpu()
        from mujoco_manip_amd import _lib

        qs = _fixture()["qpos"][_state_ids(size)]
        sim = _lib.Sim(len(qs), action_mode="abs_pos", image_size=size)
        if flags is not None:
            sim.render_effects = flags
            assert sim.render_effects == flags
        sim.reset()
        q, v, c, w = sim.get_state()
        q[:] = qs
        sim.set_state(q, v, c, w)
        sim.forward()
        torch.cuda.synchronize()
        rgb, seg = sim.image_views()
        _IMAGES[size, flags] = (rgb.cpu().numpy().copy(), seg.cpu().numpy().copy())
        sim.close()
    return _IMAGES[size, flags]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SMALL + BIG)
def test_flat_image_per_pixel(size, margin):
    """Every certain pixel of every case of the size: the reference's segment id, the colour inside the bound."""
    rgb, seg = _render(size)
    assert rgb.shape == (len(_state_ids(size)), 2, size, size, 3)
    failures = []
    for ci, cam in enumerate(CAMS):
        worst, n = 0.0, 0
        for e, i in enumerate(_state_ids(size)):
            ref = _ref(i, cam, size)
            c, rows = ref["certain"], ref["rows"]
            g_rgb, g_seg = rgb[e, ci][rows], seg[e, ci][rows]
            dist = np.abs(g_rgb.astype(float) - 255.0 * ref["f_flat"]).max(-1)
            bad_seg, bad_rgb = c & (g_seg != ref["seg"]), c & (dist > BOUND)
            n += int(c.sum())
            worst = max(worst, float(dist[c & ~bad_seg].max()))
            for what, bad in (("segment id", bad_seg), ("colour", bad_rgb & ~bad_seg)):
                for r, col in zip(*np.nonzero(bad)):
                    failures.append(f"{what}: size {size} {_fixture()['labels'][i]} {cam} row {rows[r]} col {col}: gpu seg "
                                    f"{g_seg[r, col]} rgb {g_rgb[r, col].tolist()}, reference seg {ref['seg'][r, col]} "
                                    f"255 f {np.round(255 * ref['f_flat'][r, col], 3).tolist()} face {ref['k'][r, col]}")
        print(f"size {size} {cam}: {n} certain pixels, worst |u8 - 255 f| {worst:.4f} (bound {BOUND:.4f})")
        margin(f"worst |u8 - 255 f_flat|, {size} px, {cam}", worst, BOUND, certain_pixels=n)
    assert not failures, f"{len(failures)} certain pixels differ:\n" + "\n".join(failures[:40])


@pytest.mark.gpu
@pytest.mark.parametrize("size", (128, 150))
def test_lit_kernel_at_multi_band_sizes(size):
    """The lit kernel where an image has several bands and workgroups (test_render_lit.py runs single-band sizes):
    the segment ids do not depend on the effects, and flags 0 is the flat kernel bit for bit."""
    rgb0, seg0 = _render(size)
    for flags in (0, 1, 2, 3):
        rgb, seg = _render(size, flags)
        np.testing.assert_array_equal(seg, seg0, err_msg=f"flags {flags}")
        if flags == 0:
            np.testing.assert_array_equal(rgb, rgb0)
    assert (_render(size, 3)[0] != rgb0).any()
