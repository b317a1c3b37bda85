"""Opt-in camera effects: cast shadows of the directional light and translucent bins.

CPU: the fp64 reference of the shading model (tests/render_lit_ref.py) pinned on the keyframe (floors
that keep the GPU checks from being vacuous, two hand-derived colours), the shadow map's point-to-texel
mapping on non-finite input, the two new C-ABI calls, the model tables' alphas.

GPU: 4 envs (the keyframe and three states 40 expert steps into seeded episodes, set through
set_state + forward) at 64 and 84 px: segment ids and untouched pixels bit-identical to the flat
kernel's, shadows and blends against the reference inside its certainty masks, a diverged env's poses,
the render overlap, the façades.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHADOWS, TRANSLUCENT = 1, 2
# vertices and triangles of mujoco_manip_amd/model/render_model.json before the alphas were added
GEOMETRY_SHA256 = "5a49793ea38546b2776a1abf4b6fdf1c2d2aa1843ad75ff45a317cd74171ed3c"


def _oracle_pose_fn(qpos):
    import oracle_py as O

    e = O.OracleEnv()
    e.set_state(qpos=np.asarray(qpos, float))
    e.mj_forward()
    cache = {}

    def pose(b):
        if b not in cache:
            p, R = e.body(b)
            cache[b] = (R, p)
        return cache[b]

    return pose


def _keyframe_qpos():
    m = json.load(open(os.path.join(REPO, "mujoco_manip_amd", "model", "panda_pickplace.json")))
    return np.array(m["key_qpos"], float)


_REF = {}


def _ref(key, qpos, cam, S):
    """The reference images of a state, computed once per (state, camera, size)."""
    import render_lit_ref as LR

    k = (key, cam, S)
    if k not in _REF:
        _REF[k] = LR.render(_oracle_pose_fn(qpos), cam, S)
    return _REF[k]


# ------------------------------------------------------------------------------------------ CPU
def test_reference_keyframe_floors_and_known_answers():
    """The reference alone, on the keyframe with the arm as posed: enough certain-shadow and interior
    translucent pixels for the GPU checks to mean something, at most 4 layers, and two colours derived
    by hand from DESIGN §8's formulas."""
    import render_lit_ref as LR
    import render_ref as RR

    q = _keyframe_qpos()
    w = _ref("key", q, "wrist", 64)
    o = _ref("key", q, "overhead", 96)
    n_cs, n_tr = int(w["certain_shadow"].sum()), int(LR.interior(w["translucent"]).sum())
    n_tro = int(LR.interior(o["translucent"]).sum())
    print("wrist 64: certain_shadow", n_cs, "interior translucent", n_tr, "; overhead 96: interior translucent", n_tro)
    assert n_cs >= 100
    assert n_tr >= 300
    assert n_tro >= 80
    assert w["layers"].max() <= 4 and o["layers"].max() <= 4
    # the effects change nothing else: segment ids come from the nearest surface, bins counted
    pose = _oracle_pose_fn(q)
    np.testing.assert_array_equal(w["seg"], RR.render_seg(pose, "wrist", 64))

    m = RR.model()
    mats = {x["name"]: x for x in m["materials"]}
    cR, cp = RR.camera_pose("wrist", pose)
    # 1. a table-top pixel under the hand: light 0.3 + 0.6 n_z(cam) + point term, no 0.8
    V = LR.world_vertices(pose)
    top = [k for k in range(len(m["tris"])) if m["materials"][m["tri_mat"][k]]["name"] == "table_mat"
           and np.allclose(np.cross(V[m["tris"][k, 1]] - V[m["tris"][k, 0]], V[m["tris"][k, 2]] - V[m["tris"][k, 0]])[:2], 0)
           and np.cross(V[m["tris"][k, 1]] - V[m["tris"][k, 0]], V[m["tris"][k, 2]] - V[m["tris"][k, 0]])[2] > 0]
    sel = w["certain_shadow"] & np.isin(w["k_all"], top)
    assert sel.sum() >= 20, "no table-top pixels in the hand's shadow"
    r, c = [int(x[0]) for x in np.nonzero(sel)]
    k = int(w["k_all"][r, c])
    cen = V[m["tris"][k]].mean(0)
    to_l = (LR.LIGHT_POS - cen) / np.linalg.norm(LR.LIGHT_POS - cen)
    light = 0.3 + 0.6 * cR[2, 2] + 0.4 * to_l[2]  # n = world z: n . z_cam = cR[2, 2], n . to_l = to_l[2]
    want = np.minimum(np.array(mats["table_mat"]["rgb"]) * light, 1.0)
    np.testing.assert_allclose(w["f_shadows"][r, c], want, atol=1e-12)
    np.testing.assert_allclose(w["f_flat"][r, c], np.minimum(np.array(mats["table_mat"]["rgb"]) * (light + 0.8), 1.0), atol=1e-12)
    # 2. a red-bin-bottom pixel over the table: 0.4 bin + 0.6 table, each under its own light
    red = np.array([mats[m["materials"][m["tri_mat"][k]]["name"]]["name"] == "red_bin_mat" for k in range(len(m["tris"]))])
    nz = np.cross(V[m["tris"][:, 1]] - V[m["tris"][:, 0]], V[m["tris"][:, 2]] - V[m["tris"][:, 0]])
    up = (np.abs(nz[:, :2]).max(1) < 1e-12) & (nz[:, 2] > 0)
    for ref in (o, w):
        sel = (ref["layers"] == 1) & np.isin(ref["k_all"], np.nonzero(red & up)[0]) & np.isin(ref["k_opaque"], top) & \
            ref["certain_lit_all"]
        if sel.any():
            break
    assert sel.any(), "no lit red-bin-bottom pixel over the table top"
    cRr, _ = RR.camera_pose("overhead" if ref is o else "wrist", pose)
    r, c = [int(x[0]) for x in np.nonzero(sel)]

    def face_light(k):
        cen = V[m["tris"][k]].mean(0)
        tl = (LR.LIGHT_POS - cen) / np.linalg.norm(LR.LIGHT_POS - cen)
        return 0.3 + 0.6 * max(cRr[2, 2], 0.0) + 0.8 + 0.4 * tl[2]  # horizontal faces: n = world z

    kb, kt = int(ref["k_all"][r, c]), int(ref["k_opaque"][r, c])
    want = 0.4 * np.minimum(np.array(mats["red_bin_mat"]["rgb"]) * face_light(kb), 1.0) + \
        0.6 * np.minimum(np.array(mats["table_mat"]["rgb"]) * face_light(kt), 1.0)
    np.testing.assert_allclose(ref["f_translucent"][r, c], want, atol=1e-12)
    np.testing.assert_allclose(ref["f_lit"][r, c], want, atol=1e-12)


def test_shadow_texel_mapping_on_non_finite_input():
    """The point-to-texel mapping of the shadow map (the library's own host build of the device
    function): NaN, +-Inf and +-1e30 give "outside" (-1), every finite point an index inside the map."""
    from mujoco_manip_amd import _lib

    L = _lib.load()
    L.mmx_render_shadow_texel.argtypes = [C.c_float, C.c_float]
    L.mmx_render_shadow_texel.restype = C.c_int
    L.mmx_render_shadow_map_side.restype = C.c_int
    n = L.mmx_render_shadow_map_side()
    assert 2.0 / n <= 0.008  # the texel (the map spans 2 m)
    bad = [float("nan"), float("inf"), float("-inf"), 1e30, -1e30, 3.4e38, -3.4e38]
    for b in bad:
        for other in (0.0, 0.3, b):
            assert L.mmx_render_shadow_texel(b, other) == -1
            assert L.mmx_render_shadow_texel(other, b) == -1
    rng = np.random.default_rng(0)
    for x, y in rng.uniform(-3, 3, (2000, 2)):
        k = L.mmx_render_shadow_texel(x, y)
        inside = -1.0 <= np.float32(x) < 1.0 and -0.7 <= np.float32(y) < 1.3
        assert -1 <= k < n * n
        if k >= 0:  # within a rounding of the map's square
            assert -1.0 - 1e-5 <= x <= 1.0 + 1e-5 and -0.7 - 1e-5 <= y <= 1.3 + 1e-5
        elif inside:
            assert min(abs(x + 1), abs(x - 1), abs(y + 0.7), abs(y - 1.3)) < 1e-5
    # the centre of the scene (0, 0.3) is the centre of the map; texels run along x, rows along y
    assert L.mmx_render_shadow_texel(0.0, 0.3) == (n // 2) * n + n // 2
    assert L.mmx_render_shadow_texel(-0.999, -0.699) == 0
    assert L.mmx_render_shadow_texel(0.999, 1.299) == n * n - 1


def test_render_effects_abi_without_a_sim():
    """The header declares the enum and both calls; a null sim is refused, never dereferenced."""
    from mujoco_manip_amd import _lib

    hdr = open(os.path.join(REPO, "include", "mmx_api.h")).read()
    assert "enum { MMX_RENDER_SHADOWS = 1, MMX_RENDER_TRANSLUCENT = 2 };" in hdr
    assert {"mmx_set_render_effects", "mmx_get_render_effects"} <= set(_lib.EXPORTED)
    L = _lib.load()
    assert L.mmx_set_render_effects(None, 1) == -1
    assert L.mmx_get_render_effects(None) == 0
    assert _lib.RENDER_EFFECTS == {"shadows": SHADOWS, "translucent_bins": TRANSLUCENT}
    assert _lib.render_effect_flags(()) == 0 and _lib.render_effect_flags(("shadows", "translucent_bins")) == 3
    with pytest.raises(ValueError):
        _lib.render_effect_flags(("specular",))


def test_model_tables_alpha():
    """render_model.json: the three bin materials alpha 0.4, every other 1; vertices and triangles
    are the parent commit's; the device header carries the same alphas; the bins' triangles fit the
    lit kernel's queue."""
    import re

    m = json.load(open(os.path.join(REPO, "mujoco_manip_amd", "model", "render_model.json")))
    for mat in m["materials"]:
        assert mat["alpha"] == (0.4 if mat["name"] in ("red_bin_mat", "green_bin_mat", "blue_bin_mat") else 1.0), mat
    geo = json.dumps({k: m[k] for k in ("verts", "vert_body", "tris", "tri_mat")}, separators=(",", ":"))
    assert hashlib.sha256(geo.encode()).hexdigest() == GEOMETRY_SHA256
    src = open(os.path.join(REPO, "mujoco_manip_amd", "csrc", "mmx_render_gen.h")).read()
    vals = re.search(r"MMR_mat_alpha\[(\d+)\] = \{([^}]*)\}", src)
    assert int(vals.group(1)) == len(m["materials"])
    got = [float(x.strip().rstrip("f")) for x in vals.group(2).split(",")]
    np.testing.assert_allclose(got, [x["alpha"] for x in m["materials"]], rtol=1e-7)
    nbin = sum(m["materials"][k]["alpha"] < 1.0 for k in m["tri_mat"])
    kmax = int(re.search(r"kMaxBin = (\d+);", open(os.path.join(REPO, "mujoco_manip_amd", "csrc", "mmx_render.hip")).read()).group(1))
    assert 0 < nbin <= kmax


# ------------------------------------------------------------------------------------------ GPU
def _need_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


_STATES = {}


def _states():
    """qpos [4, 30]: the keyframe and three states 40 expert steps into seeded episodes."""
    if "q" not in _STATES:
        torch = _need_gpu()
        from mujoco_manip_amd import _lib
        from mujoco_manip_amd.vec_env import PickPlaceVecEnv

        env = PickPlaceVecEnv(3, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                              image_size=0)
        env.reset(seed=[_lib.episode_seed(11, i) for i in range(3)])
        for _ in range(40):
            env.step(env.expert_plan(16))
        torch.cuda.synchronize()
        q = env.qpos.cpu().numpy().astype(np.float32)
        env.close()
        _STATES["q"] = np.concatenate([_keyframe_qpos()[None].astype(np.float32), q])
    return _STATES["q"]


_IMAGES = {}


def _render(size, flags):
    """(rgb [4, 2, S, S, 3], seg [4, 2, S, S]) of the four states; flags None: the setter never called."""
    k = (size, flags)
    if k not in _IMAGES:
        torch = _need_gpu()
        from mujoco_manip_amd import _lib

        qs = _states()
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
        _IMAGES[k] = (rgb.cpu().numpy().copy(), seg.cpu().numpy().copy())
        sim.close()
    return _IMAGES[k]


def _refs(size):
    qs = _states()
    return [[_ref(("state", i), qs[i], cam, size) for cam in ("overhead", "wrist")] for i in range(len(qs))]


def _stack(refs, name):
    return np.stack([np.stack([r[name] for r in pair]) for pair in refs])


def _within(a, b, tol):
    return (np.abs(a.astype(int) - b.astype(int)) <= tol).all(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [64, 84])
def test_segment_ids_do_not_depend_on_the_effects(size):
    _, seg0 = _render(size, None)
    for flags in (0, SHADOWS, TRANSLUCENT, SHADOWS | TRANSLUCENT):
        np.testing.assert_array_equal(_render(size, flags)[1], seg0, err_msg=f"flags {flags}")


@pytest.mark.gpu
@pytest.mark.parametrize("size", [64, 84])
def test_flag_isolation(size):
    """Flags 0 = never set; shadows only: the certainly lit pixels are the flat image's; translucency
    only: the pixels with no layer are the flat image's.  And each effect does change its pixels."""
    rgb0, _ = _render(size, None)
    np.testing.assert_array_equal(_render(size, 0)[0], rgb0)
    refs = _refs(size)
    sh = _render(size, SHADOWS)[0]
    lit = _stack(refs, "certain_lit")
    assert lit.mean() > 0.5
    np.testing.assert_array_equal(sh[lit], rgb0[lit])
    tr = _render(size, TRANSLUCENT)[0]
    none = _stack(refs, "layers") == 0
    # a silhouette pixel may show a bin on the GPU and none in the ray caster: where the GPU's own
    # segment id is a bin the pixel has a layer whatever the reference says
    seg = _render(size, None)[1]
    none &= ~np.isin(seg, (3, 4, 5))
    np.testing.assert_array_equal(tr[none], rgb0[none])
    assert (sh != rgb0).any() and (tr != rgb0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [64, 84])
def test_shadows_against_reference(size):
    """Certain-shadow pixels: the GPU colour nearer (max-channel distance) to the reference's shadowed
    image than to its flat image for at least 95 % (the margin removes texel and bias effects: what is
    left are silhouette pixels where rasteriser and ray caster hit different faces).  Certainly lit
    pixels: the flat GPU image."""
    refs = _refs(size)
    sh = _render(size, SHADOWS)[0].astype(int)
    cs = _stack(refs, "certain_shadow")
    d_lit = np.abs(sh - _stack(refs, "rgb_shadows").astype(int)).max(-1)
    d_flat = np.abs(sh - _stack(refs, "rgb_flat").astype(int)).max(-1)
    share = float((d_lit < d_flat)[cs].mean())
    print(f"size {size}: {int(cs.sum())} certain-shadow pixels, share nearer to the shadowed reference {share:.4f}")
    assert cs.sum() >= 100
    assert share >= 0.95
    lit = _stack(refs, "certain_lit")
    np.testing.assert_array_equal(_render(size, SHADOWS)[0][lit], _render(size, None)[0][lit])


@pytest.mark.gpu
@pytest.mark.parametrize("size", [64, 84])
def test_translucency_against_reference(size):
    """Interior translucent pixels whose segment id agrees with the reference: within 3 levels per
    channel of the reference blend (one for the final rounding, one per blended layer) for a share no
    lower than the flat kernel's on the same pixels against the flat reference, minus 0.02."""
    import render_lit_ref as LR

    refs = _refs(size)
    rgb0, seg = _render(size, None)
    tr = _render(size, TRANSLUCENT)[0]
    sel = np.stack([np.stack([LR.interior(r["translucent"]) for r in pair]) for pair in refs])
    sel &= seg == _stack(refs, "seg")
    flat_share = float(_within(rgb0, _stack(refs, "rgb_flat"), 3)[sel].mean())
    lit_share = float(_within(tr, _stack(refs, "rgb_translucent"), 3)[sel].mean())
    print(f"size {size}: {int(sel.sum())} interior translucent pixels, flat share {flat_share:.4f}, translucent share {lit_share:.4f}")
    assert sel.sum() >= 300
    assert lit_share >= flat_share - 0.02


@pytest.mark.gpu
@pytest.mark.parametrize("size", [64, 84])
def test_whole_image_against_reference(size):
    """All pixels, both effects on against the lit reference: the share within 3 levels is at least
    the flat mode's against the flat reference, minus 0.02."""
    refs = _refs(size)
    flat_share = float(_within(_render(size, None)[0], _stack(refs, "rgb_flat"), 3).mean())
    lit_share = float(_within(_render(size, SHADOWS | TRANSLUCENT)[0], _stack(refs, "rgb_lit"), 3).mean())
    print(f"size {size}: whole image, flat share {flat_share:.4f}, lit share {lit_share:.4f}")
    assert lit_share >= flat_share - 0.02


@pytest.mark.gpu
def test_set_render_effects_errors():
    _need_gpu()
    from mujoco_manip_amd import _lib

    sim = _lib.Sim(2, action_mode="abs_pos", image_size=64)
    assert sim.L.mmx_set_render_effects(sim.ptr, 4) == -1
    assert sim.L.mmx_set_render_effects(sim.ptr, -1) == -1
    assert sim.render_effects == 0
    sim.render_effects = ("shadows",)
    assert sim.render_effects == SHADOWS
    sim.render_effects = 0
    assert sim.render_effects == 0
    sim.close()
    nocam = _lib.Sim(2, action_mode="abs_pos", image_size=0)
    assert nocam.L.mmx_set_render_effects(nocam.ptr, 1) == -1
    assert nocam.L.mmx_set_render_effects(nocam.ptr, 0) == -1
    nocam.close()
    with pytest.raises(ValueError):
        _lib.Sim(2, action_mode="abs_pos", image_size=0, render_effects=("shadows",))


@pytest.mark.gpu
def test_two_live_sims_keep_their_own_effects():
    """Every render launch gets its sim's flags and shadow maps as arguments: two live sims of the four
    states at 64 px, A with both effects and B with none, rendered in turn (A, B, A again) give the images
    of the sims that had the device to themselves, bit for bit; closing A leaves B's render unchanged, and
    B set to shadows afterwards renders as a sim that had shadows from the start."""
    torch = _need_gpu()
    from mujoco_manip_amd import _lib

    qs = _states()

    def make(flags):
        sim = _lib.Sim(len(qs), action_mode="abs_pos", image_size=64)
        if flags is not None:
            sim.render_effects = flags
        sim.reset()
        q, v, c, w = sim.get_state()
        q[:] = qs
        sim.set_state(q, v, c, w)
        return sim

    def images(sim):
        sim.forward()
        torch.cuda.synchronize()
        rgb, seg = sim.image_views()
        return rgb.cpu().numpy().copy(), seg.cpu().numpy().copy()

    def same(got, want, msg):
        np.testing.assert_array_equal(got[0], want[0], err_msg=msg + ": rgb")
        np.testing.assert_array_equal(got[1], want[1], err_msg=msg + ": seg")

    a, b = make(SHADOWS | TRANSLUCENT), make(None)
    same(images(a), _render(64, SHADOWS | TRANSLUCENT), "A first")
    same(images(b), _render(64, None), "B after A")
    same(images(a), _render(64, SHADOWS | TRANSLUCENT), "A after B")
    a.close()
    same(images(b), _render(64, None), "B after A closed")
    b.render_effects = SHADOWS
    assert b.render_effects == SHADOWS
    same(images(b), _render(64, SHADOWS), "B set to shadows")
    b.close()
    assert (_render(64, SHADOWS | TRANSLUCENT)[0] != _render(64, None)[0]).any()


@pytest.mark.gpu
def test_render_overlap_bit_identical_with_effects(monkeypatch):
    """MMX_RENDER_OVERLAP 0 and 1 with both effects: the shadow pass runs on the render's stream and
    pose buffer, so the images after 5 and then 2 more rollout steps are the same bit for bit."""
    torch = _need_gpu()
    from mujoco_manip_amd import _lib
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    N, S = 64, 64
    outs = []
    for ov in ("0", "1"):
        monkeypatch.setenv("MMX_RENDER_OVERLAP", ov)
        env = PickPlaceVecEnv(N, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                              image_size=S, autoreset=True, render_effects=("shadows", "translucent_bins"))
        assert env.sim.rollout_render_overlap == (ov == "1")
        env.reset(seed=[_lib.episode_seed(5, i) for i in range(N)])
        got = []
        for n in (5, 2):
            env.rollout_expert(n)
            torch.cuda.synchronize()
            rgb, seg = env.sim.image_views()
            got += [rgb.cpu().numpy().copy(), seg.cpu().numpy().copy()]
        outs.append(got)
        env.close()
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    assert (outs[0][0] != outs[0][2]).any()  # the scene moved between the two read-outs


@pytest.mark.gpu
def test_facade_and_dataset_record_the_option(tmp_path):
    torch = _need_gpu()
    from mujoco_manip_amd import dataset
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    imgs = []
    for fx in ((), ("shadows", "translucent_bins")):
        env = PickPlaceVecEnv(1, task=("obj_red", "bin_blue"), action_mode="abs_pos", image_size=64, render_effects=fx)
        obs, _ = env.reset(seed=0)
        torch.cuda.synchronize()
        imgs.append(obs["image_wrist"].cpu().numpy().copy())
        env.close()
    assert imgs[0].shape == (1, 64, 64, 3) and (imgs[0] != imgs[1]).any()
    out, _ = dataset.generate("t/lit", num_episodes=2, root=str(tmp_path), task=("obj_red", "bin_blue"), num_envs=2, image_size=64,
                              render_effects=("shadows", "translucent_bins"))
    md = json.load(open(os.path.join(out, "metadata.json")))
    assert md["render_effects"] == ["shadows", "translucent_bins"] and md["image_size"] == 64
    out0, _ = dataset.generate("t/flat", num_episodes=2, root=str(tmp_path), task=("obj_red", "bin_blue"), num_envs=2, image_size=64)
    assert "render_effects" not in json.load(open(os.path.join(out0, "metadata.json")))


@pytest.mark.gpu
def test_render_after_divergence_with_effects():
    """A diverged env's NaN / Inf poses reach the shadow pass and the lit kernel when autoreset is off
    (the procedure of test_render.py::test_render_after_divergence_without_autoreset, both effects on):
    the injected envs are flagged, the others' images equal an uninjected run's bit for bit (the shadow
    pass culls by the integer-bit area test and clamps every texel index), segment ids stay valid."""
    torch = _need_gpu()
    from mujoco_manip_amd import _lib
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    outs = []
    for inject in (False, True):
        env = PickPlaceVecEnv(4, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                              image_size=64, autoreset=False, render_effects=("shadows", "translucent_bins"))
        env.reset(seed=[_lib.episode_seed(13, i) for i in range(4)])
        if inject:
            q, v, c, w = env.sim.get_state()
            v[1, 3] = np.nan
            v[2, 0] = np.inf
            env.sim.set_state(q, v, c, w)
        for _ in range(2):
            obs, *_ = env.step(env.expert_plan(16))
        torch.cuda.synchronize()
        outs.append((obs["image_overhead"].cpu().numpy(), obs["image_wrist"].cpu().numpy(),
                     env.segmentation.cpu().numpy(), env.env_error.cpu().numpy()))
        env.close()
    (o0, w0, s0, e0), (o1, w1, s1, e1) = outs
    assert (e0 == 0).all()
    assert e1[1] != 0 and e1[2] != 0 and e1[0] == 0 and e1[3] == 0, e1
    for k in (0, 3):
        np.testing.assert_array_equal(o1[k], o0[k])
        np.testing.assert_array_equal(w1[k], w0[k])
        np.testing.assert_array_equal(s1[k], s0[k])
    assert s1.max() <= 9
