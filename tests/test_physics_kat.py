"""Known-answer scenes that pin the physics to MuJoCo's published constraint model, independently
of both implementations (VERDICT r02 "next" #2).

The reference's physics is mujoco==3.5.0's mj_step (env.py:119-121), un-vendored and absent from
this image; the reference tests pin only behavioural thresholds.  Each scene below has
an answer derived in this file from the equations MuJoCo publishes (documentation, "Computation"
chapter: soft constraints, impedance, reference acceleration, pyramidal cones; "Modeling": contact
parameter mixing), not from the oracle's or the kernel's code.  The same scenes run through the
fp64 oracle (CPU tests, `oracle/`) and through the HIP kernel (`-m gpu`, mmx_physics_step through
the C-ABI), so an error in the shared modelling assumptions (regulariser R, aref, impedance,
pyramid edges, free-joint integration) fails here even though the GPU-vs-oracle tests would pass.

Equations (MuJoCo documentation, Computation / Soft constraints, with this model's values):
  * impedance d(r) from solimp = (dmin, dmax, width, mid, power) = (0.9, 0.95, 0.001, 0.5, 2):
    x = |r| / width; y = x^p / mid^(p-1) for x <= mid, 1 - (1-x)^p / (1-mid)^(p-1) above, y = 1 for
    x >= 1; d = dmin + y (dmax - dmin);
  * reference acceleration aref = -b (J v) - k d r with b = 2 / (dmax tau), k = 1 / (dmax^2 tau^2
    zeta^2), solref = (tau, zeta) = (0.02, 1) (tau >= 2 timestep);
  * regulariser R = (1 - d) / d * A_hat with A_hat the diagonal approximation; for a pyramidal
    contact every edge shares A_hat = 2 mu0^2 (t + mu0^2 t) / impratio, t = the two bodies'
    translational invweight0 (1 / m = 20 for a free 0.05 kg cube, 0 for the static table),
    impratio = 1 (the model sets none);
  * pyramid edges of a condim-4 contact: J_n +- mu_k J_k for the two tangents (mu = 2) and the
    rotation about the normal (mu = 1): contact friction (2, 2, 1) = elementwise max of the cube's
    (2, 1, 0.01) and the table's default (1, 0.005, 0.0001), expanded (slide, slide, spin);
  * primal problem: qacc minimises 1/2 (a - a0)' M (a - a0) + sum over active edges of
    1/2 D (J a - aref)^2, D = 1 / R; an edge is active when J a < aref;
  * free joint: linear velocity in the world frame, angular velocity in the body frame,
    quaternion q <- q (x) exp(omega h / 2); semi-implicit Euler v <- v + h a, x <- x + h v.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

H = 0.002
G = 9.81
M_CUBE = 0.05
HALF = 0.02
TRAN = 1.0 / M_CUBE
MU = (2.0, 2.0, 1.0)
SOLIMP = (0.9, 0.95, 0.001, 0.5, 2.0)
TAU, ZETA = 0.02, 1.0
TABLE_TOP = 0.24
RED, GREEN, BLUE = 0, 1, 2


def impedance(r):
    dmin, dmax, width, mid, p = SOLIMP
    x = abs(r) / width
    if x >= 1.0:
        return dmax
    y = x ** p / mid ** (p - 1) if x <= mid else 1.0 - (1.0 - x) ** p / (1.0 - mid) ** (p - 1)
    return dmin + y * (dmax - dmin)


def kb():
    dmax = SOLIMP[1]
    return 1.0 / (dmax * dmax * TAU * TAU * ZETA * ZETA), 2.0 / (dmax * TAU)


def a_hat_pyramid(tran=TRAN, mu0=MU[0], impratio=1.0):
    return 2.0 * mu0 * mu0 * (tran + mu0 * mu0 * tran) / impratio


def rest_penetration(ncon, a_hat=None, edges=6, load=M_CUBE * G, tran=TRAN):
    """Penetration r < 0 at which `ncon` equal contacts carry `load` (by default a resting cube's
    weight on its corner contacts): with v = 0 and qacc = 0 every edge is active and pushes
    D aref = k d(r)^2 |r| / ((1 - d) A_hat) along the normal, so ncon * edges * that = load.  `tran`
    is the sum of the two bodies' translational invweight0 in A_hat (20 for a cube on the static
    table, 20 + 20 for a cube on a cube).  Solved by bisection (monotone in |r|)."""
    K, _ = kb()
    A = a_hat_pyramid(tran) if a_hat is None else a_hat

    def total(p):
        d = impedance(p)
        return ncon * edges * K * d * d * p / ((1.0 - d) * A)

    lo, hi = 0.0, 0.01
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if total(mid) < load:
            lo = mid
        else:
            hi = mid
    return -0.5 * (lo + hi)


def make_frame(n):
    """mju_makeFrame: the contact's tangents from its normal."""
    n = np.asarray(n, float) / np.linalg.norm(n)
    y = np.array([0.0, 1.0, 0.0]) if -0.5 < n[1] < 0.5 else np.array([0.0, 0.0, 1.0])
    t1 = y - n * n.dot(y)
    t1 /= np.linalg.norm(t1)
    return np.stack([n, t1, np.cross(n, t1)])


def first_step_velocity(com, v6, contacts):
    """Exact qvel after one substep of a free cube (unrotated, isotropic inertia) on the static
    table, from the primal problem with every pyramid edge active (checked afterwards).
    v6 = (linear world, angular body); contacts = [(pos, normal pointing into the cube, dist)]."""
    K, B = kb()
    I = M_CUBE * (2 * HALF) ** 2 / 6.0
    Mm = np.diag([M_CUBE] * 3 + [I] * 3)
    a0 = np.array([0.0, 0.0, -G, 0.0, 0.0, 0.0])
    A = Mm.copy()
    rhs = Mm @ a0
    rows = []
    for pos, n, dist in contacts:
        F = make_frame(n)
        r = np.asarray(pos) - com
        Jn = np.r_[F[0], np.cross(r, F[0])]
        Jk = [np.r_[F[1], np.cross(r, F[1])], np.r_[F[2], np.cross(r, F[2])], np.r_[np.zeros(3), F[0]]]
        d = impedance(dist)
        D = 1.0 / ((1.0 - d) / d * a_hat_pyramid())
        for k in range(3):
            for sg in (1.0, -1.0):
                J = Jn + sg * MU[k] * Jk[k]
                aref = -B * J.dot(v6) - K * d * dist
                A += D * np.outer(J, J)
                rhs += D * aref * J
                rows.append((J, aref))
    acc = np.linalg.solve(A, rhs)
    assert all(J.dot(acc) < aref for J, aref in rows), "not every edge active: closed form invalid"
    return v6 + H * acc


def _cube(q, o):
    return q[9 + 7 * o: 12 + 7 * o], q[12 + 7 * o: 16 + 7 * o]


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def free_fall_answer(x0, v0, w_body, q0, n):
    """Semi-implicit Euler under gravity (exact recurrence) and constant body-frame spin."""
    z = x0[2] + n * H * v0[2] - G * H * H * n * (n + 1) / 2.0
    pos = np.array([x0[0] + n * H * v0[0], x0[1] + n * H * v0[1], z])
    vel = np.array([v0[0], v0[1], v0[2] - n * G * H])
    wn = np.linalg.norm(w_body)
    ang = wn * H * n
    q = _qmul(q0, np.r_[np.cos(ang / 2), np.sin(ang / 2) * np.asarray(w_body) / wn])
    return pos, vel, q


FALL_X0 = np.array([0.6, -0.4, 1.0])
FALL_V0 = np.array([0.1, -0.05, 1.5])
FALL_W = np.array([3.0, -2.0, 5.0])
FALL_Q0 = np.array([np.cos(0.3), 0.0, np.sin(0.3), 0.0])
FALL_N = 200


def test_rest_closed_form_discriminates_regularisers():
    """The rest-penetration answer depends on the regulariser: MuJoCo's common pyramidal A_hat
    (800 here) against the per-edge diagApprox (t + mu_k^2 t = 100 for the sliding edges, the
    round-1 form) differ by several times the tolerances used below."""
    p_common = rest_penetration(4)
    p_edge = rest_penetration(4, a_hat=TRAN + MU[0] ** 2 * TRAN)
    assert -6e-4 < p_common < -4e-4, p_common
    assert abs(p_common - p_edge) > 2e-4, (p_common, p_edge)
    # the answer carries the cube: 24 edges x D aref = m g
    K, _ = kb()
    d = impedance(p_common)
    assert abs(24 * K * d * d * -p_common / ((1 - d) * a_hat_pyramid()) - M_CUBE * G) < 1e-9


# --------------------------------------------------------------------------- oracle (CPU)
def _oracle_settled(n=500):
    import oracle_py as O

    e = O.OracleEnv()
    e.reset_keyframe()
    for _ in range(n):
        e.mj_step()
    return e


def test_oracle_rest_penetration_and_R():
    """Three cubes resting on the table (keyframe, 1 s): each sits 4 corner contacts deep at the
    closed-form penetration, is at rest, and every contact edge's R equals the published
    pyramidal formula at that depth."""
    e = _oracle_settled()
    q, v, _, _ = e.get_state()
    cons = e.contacts()
    for o in (RED, GREEN, BLUE):
        pos, quat = _cube(q, o)
        mine = [c for c in cons if np.linalg.norm(c["pos"][:2] - pos[:2]) < 0.03 and abs(c["pos"][2] - TABLE_TOP) < 0.01]
        assert len(mine) == 4, (o, len(mine))
        p = rest_penetration(len(mine))
        for c in mine:
            assert abs(c["dist"] - p) < 2e-8, (o, c["dist"], p)
        assert abs(pos[2] - (TABLE_TOP + HALF + p)) < 2e-8, (o, pos[2])
        np.testing.assert_allclose(v[9 + 6 * o: 15 + 6 * o], 0.0, atol=1e-9)
    efc = e.efc()
    rows = efc["type"] == 2
    assert rows.sum() == 12 * 6
    for pos, R in zip(efc["pos"][rows], efc["R"][rows]):
        d = impedance(pos)
        assert abs(R - (1 - d) / d * a_hat_pyramid()) < 1e-9 * R, (pos, R)


def test_oracle_free_fall_exact():
    """Red cube thrown up with a body-frame spin, far from everything: 200 substeps follow the
    semi-implicit Euler recurrence and the body-frame quaternion exponential exactly."""
    import oracle_py as O

    e = O.OracleEnv()
    e.reset_keyframe()
    q, v, c, w = e.get_state()
    q[9:12], q[12:16] = FALL_X0, FALL_Q0
    v[9:12], v[12:15] = FALL_V0, FALL_W
    e.set_state(q, v, c, w)
    for _ in range(FALL_N):
        e.mj_step()
    q, v, _, _ = e.get_state()
    pos, vel, quat = free_fall_answer(FALL_X0, FALL_V0, FALL_W, FALL_Q0, FALL_N)
    np.testing.assert_allclose(q[9:12], pos, atol=1e-12)
    np.testing.assert_allclose(v[9:12], vel, atol=1e-12)
    np.testing.assert_allclose(v[12:15], FALL_W, atol=1e-12)
    np.testing.assert_allclose(q[12:16] * np.sign(q[12]), quat * np.sign(quat[0]), atol=1e-10)


def _oracle_cube_contacts(e, o):
    q = e.get_state()[0]
    pos, _ = _cube(q, o)
    out = []
    for c in e.contacts():
        if np.linalg.norm(c["pos"][:2] - pos[:2]) < 0.03 and abs(c["pos"][2] - TABLE_TOP) < 0.01:
            n = c["frame"][0] * np.sign(c["frame"][0][2])  # normal pointing into the cube
            out.append((c["pos"], n, c["dist"]))
    return out


def test_oracle_slide_first_step_closed_form():
    """A resting cube given a slow push (0.02 m/s along x, inside the pyramid: every edge stays
    active): one substep gives the velocity of the closed-form primal solution (6-dof free body,
    24 pyramid edges, common R, aref with the velocity term)."""
    e = _oracle_settled()
    q, v, c, w = e.get_state()
    com = _cube(q, RED)[0].copy()
    cons = _oracle_cube_contacts(e, RED)
    assert len(cons) == 4
    v = v.copy()
    v[9] = 0.02
    e.set_state(q, v, c, w)
    v6 = v[9:15].copy()
    e.mj_step()
    want = first_step_velocity(com, v6, cons)
    got = e.get_state()[1][9:15]
    np.testing.assert_allclose(got, want, atol=1e-9)
    assert 0.78 < got[0] / v6[0] < 0.86  # friction damps the slide by ~17 % per substep


def test_oracle_slide_coulomb_bound():
    """A fast push (0.5 m/s): the pyramid's edge forces are non-negative, so per substep the
    friction the cube feels is at most mu times the normal force it feels:
    |m a_x| <= mu m (a_z + g) (the table is the only thing touching it)."""
    e = _oracle_settled()
    q, v, c, w = e.get_state()
    v = v.copy()
    v[9] = 0.5
    e.set_state(q, v, c, w)
    prev = v[9:12].copy()
    for _ in range(40):
        e.mj_step()
        cur = e.get_state()[1][9:12].copy()
        ax, az = (cur[0] - prev[0]) / H, (cur[2] - prev[2]) / H
        assert abs(ax) <= MU[0] * (az + G) + 1e-6, (ax, az)
        prev = cur


# --------------------------------------------------------------------------- GPU (HIP kernel)
def _gpu_sim(rows, n=1):
    from mujoco_manip_amd import _lib

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    sim = _lib.Sim(n, action_mode="abs_pos", image_size=0)
    sim.reset()  # keyframe (no randomisation)
    sim.step_rows = rows
    assert sim.step_rows == rows
    return sim


def _gpu_contacts(sim, env=0):
    from mujoco_manip_amd import _lib

    ncon = int(sim.view("episode_i", _lib.EPI_N, "<i4")[env, _lib.EPI["ncon"]].item())
    con = sim.view("contacts", _lib.MAXCON * _lib.CON_F).cpu().numpy()[env].reshape(_lib.MAXCON, _lib.CON_F)[:ncon]
    return con


def _test_gpu_rest_penetration(rows):
    """The kernel's resting cubes (keyframe, 1 s = 500 substeps) against the closed form."""
    sim = _gpu_sim(rows)
    sim.physics_step(500, with_ik=False)
    q, v, _, _ = sim.get_state()
    con = _gpu_contacts(sim)
    for o in (RED, GREEN, BLUE):
        pos, _ = _cube(q[0], o)
        mine = [c for c in con if np.linalg.norm(c[1:3] - pos[:2]) < 0.03 and abs(c[3] - TABLE_TOP) < 0.01]
        assert len(mine) == 4, (o, len(mine))
        p = rest_penetration(len(mine))
        for c in mine:
            assert abs(c[0] - p) < 2e-6, (o, float(c[0]), p)  # fp32: 0.26 m at ~3e-8
        assert abs(pos[2] - (TABLE_TOP + HALF + p)) < 2e-6, (o, float(pos[2]), p)
        assert np.abs(v[0, 9 + 6 * o: 15 + 6 * o]).max() < 1e-4
    sim.close()


def _test_gpu_free_fall_exact(rows):
    sim = _gpu_sim(rows)
    q, v, c, w = sim.get_state()
    q[0, 9:12], q[0, 12:16] = FALL_X0, FALL_Q0
    v[0, 9:12], v[0, 12:15] = FALL_V0, FALL_W
    sim.set_state(q, v, c, w)
    sim.physics_step(FALL_N, with_ik=False)
    q, v, _, _ = sim.get_state()
    pos, vel, quat = free_fall_answer(FALL_X0, FALL_V0, FALL_W, FALL_Q0, FALL_N)
    np.testing.assert_allclose(q[0, 9:12], pos, atol=2e-5)  # fp32 accumulation over 200 substeps
    np.testing.assert_allclose(v[0, 9:12], vel, atol=1e-5)
    np.testing.assert_allclose(v[0, 12:15], FALL_W, atol=1e-5)
    np.testing.assert_allclose(q[0, 12:16] * np.sign(q[0, 12]), quat * np.sign(quat[0]), atol=1e-4)
    sim.close()


def _test_gpu_slide_first_step_closed_form(rows):
    sim = _gpu_sim(rows)
    sim.physics_step(500, with_ik=False)
    q, v, c, w = sim.get_state()
    com = _cube(q[0], RED)[0].astype(float)
    cons = []
    for cc in _gpu_contacts(sim):
        if np.linalg.norm(cc[1:3] - com[:2]) < 0.03 and abs(cc[3] - TABLE_TOP) < 0.01:
            n = cc[4:7].astype(float)
            cons.append((cc[1:4].astype(float), n * np.sign(n[2]), float(cc[0])))
    assert len(cons) == 4
    v[0, 9:15] = [0.02, 0, 0, 0, 0, 0]
    sim.set_state(q, v, c, w)
    sim.physics_step(1, with_ik=False)
    got = sim.get_state()[1][0, 9:15]
    want = first_step_velocity(com, np.array([0.02, 0, 0, 0, 0, 0]), cons)
    np.testing.assert_allclose(got, want, atol=2e-5)  # 0.1 % of the push
    sim.close()


def _test_gpu_slide_coulomb_bound_and_oracle(rows):
    """The fast push on the device: the Coulomb bound per substep, and the trajectory (a hop and a
    tip: mu = 2 > half-width / half-height) within 1 mm of the oracle's over 40 substeps."""
    import oracle_py as O

    sim = _gpu_sim(rows)
    sim.physics_step(500, with_ik=False)
    q, v, c, w = sim.get_state()
    v[0, 9] = 0.5
    sim.set_state(q, v, c, w)
    e = O.OracleEnv()
    e.set_state(q[0].astype(float), v[0].astype(float), c[0].astype(float), w[0].astype(float))
    e.mj_forward()
    prev = v[0, 9:12].astype(float)
    for k in range(40):
        sim.physics_step(1, with_ik=False)
        e.mj_step()
        gq, gv, _, _ = sim.get_state()
        cur = gv[0, 9:12].astype(float)
        ax, az = (cur[0] - prev[0]) / H, (cur[2] - prev[2]) / H
        assert abs(ax) <= MU[0] * (az + G) + 5e-3, (k, ax, az)  # fp32 velocities: 1e-5 / h
        prev = cur
        rq = e.get_state()[0]
        assert np.abs(gq[0, 9:16] - rq[9:16]).max() < 1e-3, (k, gq[0, 9:16], rq[9:16])
    sim.close()


# Each physics-level test on both step layouts: physics_step runs the one-substep kernel of the sim's layout.
# The test of the 128-row single-wave kernel keeps its name; _l192 is the 192-row kernel with its helper wave.

@pytest.mark.gpu
def test_gpu_rest_penetration():
    _test_gpu_rest_penetration(rows=128)


@pytest.mark.gpu
def test_gpu_rest_penetration_l192():
    _test_gpu_rest_penetration(rows=192)


@pytest.mark.gpu
def test_gpu_free_fall_exact():
    _test_gpu_free_fall_exact(rows=128)


@pytest.mark.gpu
def test_gpu_free_fall_exact_l192():
    _test_gpu_free_fall_exact(rows=192)


@pytest.mark.gpu
def test_gpu_slide_first_step_closed_form():
    _test_gpu_slide_first_step_closed_form(rows=128)


@pytest.mark.gpu
def test_gpu_slide_first_step_closed_form_l192():
    _test_gpu_slide_first_step_closed_form(rows=192)


@pytest.mark.gpu
def test_gpu_slide_coulomb_bound_and_oracle():
    _test_gpu_slide_coulomb_bound_and_oracle(rows=128)


@pytest.mark.gpu
def test_gpu_slide_coulomb_bound_and_oracle_l192():
    _test_gpu_slide_coulomb_bound_and_oracle(rows=192)
