"""FrankaCubeLift-v0, CPU side: the oracle's independent restatement of the reference's term functions against
the fixture generated from the reference's own torch code, and plausibility of the reduced arm / cube / gripper model (no
physics oracle exists: PhysX; parity of that layer is unpinned)."""
import numpy as np
import pytest

from helpers import assert_close


@pytest.fixture(scope="module")
def lo():
    from oracle import lift_oracle
    lift_oracle.build()
    lift_oracle.lib()
    return lift_oracle


def test_lift_terms_golden(lo, golden_dir):
    """rewards.py:20-67 (object_is_lifted, object_ee_distance, object_goal_distance x 2 stds) and observations.py:19-31
    (object_position_in_robot_root_frame): 192 rows incl. the 0.06 m threshold from both sides and arbitrary root poses."""
    g = np.load(f"{golden_dir}/lift_terms.npz")
    lifted, reach, goal, fine, pos_b = lo.terms(g["object_pos_w"], g["ee_pos_w"], g["robot_root_state_w"], g["command"])
    assert_close(lifted, g["rew_object_is_lifted"], 0, 0, "object_is_lifted")
    assert_close(reach, g["rew_object_ee_distance"], 3e-7, 2e-6, "object_ee_distance (tanh kernel)")
    assert_close(goal, g["rew_object_goal_distance_03"], 3e-7, 2e-6, "object_goal_distance std 0.3")
    assert_close(fine, g["rew_object_goal_distance_005"], 3e-7, 2e-6, "object_goal_distance std 0.05")
    assert_close(pos_b, g["obs_object_position_in_robot_root_frame"], 3e-7, 2e-6, "object_position_in_robot_root_frame")
    assert lifted[:3].tolist() == [0.0, 1.0, 0.0]                 # z = 0.06 (not >), 0.0600001, 0.0599999


def test_tanh_and_model_kinematics(lo):
    x = np.linspace(-9, 9, 4001).astype(np.float32)
    t = np.array([lo.lib().lfo_tanhf(float(v)) for v in x], np.float32)
    assert np.abs(t - np.tanh(x.astype(np.float64))).max() < 2e-7
    cfg = lo.default_config()
    tcp, R, v, w = lo.hand_pose(cfg, lo.Q_DEFAULT)
    assert abs(tcp[1]) < 1e-6 and 0.40 < tcp[0] < 0.52 and 0.30 < tcp[2] < 0.48      # home pose: in front of the base, above the table
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-6) and abs(np.linalg.det(R) - 1) < 1e-5
    # hand twist = numerical derivative of the pose
    rng = np.random.RandomState(0)
    q = lo.Q_DEFAULT.copy()
    q[:7] += rng.uniform(-0.3, 0.3, 7)
    qd = np.zeros(9, np.float32)
    qd[:7] = rng.uniform(-1, 1, 7)
    tcp0, R0, v, w = lo.hand_pose(cfg, q, qd)
    eps = 1e-3
    tcp1, R1, _, _ = lo.hand_pose(cfg, q + eps * qd)
    assert np.allclose((tcp1 - tcp0) / eps, v, atol=3e-3)
    dR = (R1 - R0) / eps @ R0.T
    assert np.allclose([dR[2, 1], dR[0, 2], dR[1, 0]], w, atol=5e-3)


def test_arm_dynamics_are_consistent(lo):
    """Mass matrix symmetric positive definite; gravity torque = gradient of the potential energy (checked through the
    torque-free equilibrium droop: stiffness 80 N m / rad holds the home pose within tau_g / 80)."""
    rng = np.random.RandomState(1)
    for _ in range(5):
        q = (lo.Q_DEFAULT[:7] + rng.uniform(-0.5, 0.5, 7)).astype(np.float32)
        M = lo.mass_matrix(q)
        assert np.abs(M - M.T).max() < 1e-5 and np.linalg.eigvalsh((M + M.T) / 2).min() > 1e-3
    cfg = lo.default_config()
    S = lo.new_state(2)
    lo.reset(cfg, S)
    a = np.zeros((2, 8), np.float32)
    for _ in range(150):
        lo.step(cfg, S, a)
    droop = S[0, :7] - lo.Q_DEFAULT[:7]
    tau_g = lo.gravity_torque(S[0, :7])
    assert np.abs(S[0, 9:16]).max() < 0.02, "arm at rest"
    assert np.allclose(80.0 * (-droop), tau_g, atol=0.6), (droop, tau_g)      # PD torque balances gravity
    assert np.abs(droop).max() < 0.35


def test_cube_rests_slides_and_is_grasped(lo):
    cfg = lo.default_config()
    S = lo.new_state(1)
    lo.reset(cfg, S)
    a = np.zeros((1, 8), np.float32)
    for _ in range(60):
        lo.step(cfg, S, a)
    assert abs(S[0, lo.OBJ_POS + 2] - 0.02) < 5e-4 and np.abs(S[0, lo.OBJ_LIN:lo.OBJ_LIN + 6]).max() < 1e-2   # at rest on the table
    # Coulomb friction: a horizontal push decays at mu g
    S[0, lo.OBJ_LIN] = 0.6
    x0 = S[0, lo.OBJ_POS]
    for _ in range(25):
        lo.step(cfg, S, a)
    travelled = S[0, lo.OBJ_POS] - x0
    assert abs(travelled - 0.6 ** 2 / (2 * cfg.mu_table * 9.81)) < 0.012 and abs(S[0, lo.OBJ_LIN]) < 1e-2
    # grasp: put the cube between the open fingers at the tool centre point, close, it stays in the hand
    S2 = lo.new_state(1)
    lo.reset(cfg, S2)
    for _ in range(100):
        lo.step(cfg, S2, a)
    tcp, R, _, _ = lo.hand_pose(cfg, S2[0, :9])
    S2[0, lo.OBJ_POS:lo.OBJ_POS + 3] = tcp
    S2[0, lo.OBJ_LIN:lo.OBJ_LIN + 6] = 0
    S2[0, 7:9] = 0.0205                           # pads just off the faces (closing takes 0.1 s at 0.2 m/s: the cube would drop)
    close = a.copy()
    close[0, 7] = -1.0
    for _ in range(100):
        lo.step(cfg, S2, close)
    tcp2, _, _, _ = lo.hand_pose(cfg, S2[0, :9])
    assert np.linalg.norm(S2[0, lo.OBJ_POS:lo.OBJ_POS + 3] - tcp2) < 0.012, "the cube is held between the pads"
    assert S2[0, 7] < 0.03 and S2[0, 8] < 0.03 and S2[0, 7] > 0.012        # fingers stopped by the cube (half width 0.02)
    assert S2[0, lo.OBJ_POS + 2] > 0.2
    # without closing it falls to the table
    S3 = S2.copy()
    S3[0, 7:9] = 0.04
    for _ in range(100):
        lo.step(cfg, S3, a)
    assert S3[0, lo.OBJ_POS + 2] < 0.05


def test_lift_mdp_ordering_and_resets(lo):
    cfg = lo.default_config()
    n = 64
    S = lo.new_state(n)
    obs = lo.reset(cfg, S)
    assert obs.shape == (n, 36) and np.abs(obs[:, :18]).max() == 0          # default pose, zero velocities
    assert np.allclose(obs[:, 18:21], S[:, lo.OBJ_POS:lo.OBJ_POS + 3]) and (obs[:, 24] == 1).all()
    assert (S[:, lo.OBJ_POS] >= 0.4 - 1e-6).all() and (S[:, lo.OBJ_POS] <= 0.6 + 1e-6).all()
    assert (np.abs(S[:, lo.OBJ_POS + 1]) <= 0.25 + 1e-6).all() and (S[:, lo.CMD] >= 0.3).all() and (S[:, lo.CMD] <= 0.7).all()
    rng = np.random.RandomState(0)
    log = np.zeros(16, np.float32)
    trunc_seen = 0
    for k in range(252):
        a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        obs, r, term, trunc, log = lo.step(cfg, S, a, log=log)
        assert np.isfinite(obs).all() and np.isfinite(r).all()
        trunc_seen += int(trunc.sum())
        if k < 249:
            assert trunc.sum() == 0
            assert np.array_equal(obs[~term.astype(bool), 28:36], a[~term.astype(bool)])       # last_action of non-reset envs
    assert trunc_seen >= n - 8                                    # 5 s episodes: everybody times out at step 250
    assert log[8] >= 0 and np.isfinite(log[:8]).all()
    ep = S[:, lo.EP_LEN].view(np.int32)
    assert ep.max() <= 2


def _panda_lagrangian(q, params):
    """Independent float64 restatement of the arm's rigid-body dynamics from the SAME published parameters (modified-DH
    table, link masses / centres of mass / principal inertias -- data, restated here) by the Lagrangian route: link frames
    by homogeneous transforms, geometric Jacobians of every centre of mass, M = sum m Jv^T Jv + Jw^T (R I R^T) Jw and the
    potential energy.  Nothing of lift_model.h's recursive Newton-Euler code is shared."""
    A, D, alpha, m, Cm, Ii = params
    T = np.eye(4)
    Rs, os_, zs = [], [], []
    for i in range(7):
        ca, sa, ct, st = np.cos(alpha[i]), np.sin(alpha[i]), np.cos(q[i]), np.sin(q[i])
        Ti = np.array([[ct, -st, 0.0, A[i]],
                       [st * ca, ct * ca, -sa, -sa * D[i]],
                       [st * sa, ct * sa, ca, ca * D[i]],
                       [0.0, 0.0, 0.0, 1.0]])
        T = T @ Ti
        Rs.append(T[:3, :3].copy()); os_.append(T[:3, 3].copy()); zs.append(T[:3, 2].copy())
    M = np.zeros((7, 7))
    U = 0.0
    for i in range(7):
        c = os_[i] + Rs[i] @ Cm[i]
        Jv, Jw = np.zeros((3, 7)), np.zeros((3, 7))
        for j in range(i + 1):
            Jv[:, j] = np.cross(zs[j], c - os_[j])
            Jw[:, j] = zs[j]
        Iw = Rs[i] @ np.diag(Ii[i]) @ Rs[i].T
        M += m[i] * Jv.T @ Jv + Jw.T @ Iw @ Jw
        U += m[i] * 9.81 * c[2]
    return M, U


def test_arm_dynamics_match_an_independent_lagrangian_restatement(lo):
    """lm_rne (recursive Newton-Euler, float32) against a float64 Lagrangian restatement: mass matrix, gravity torque =
    dU/dq, and the velocity terms c(q, qd) = Mdot qd - 1/2 d(qd^T M qd)/dq, at random configurations."""
    params = (np.array([0.0, 0.0, 0.0, 0.0825, -0.0825, 0.0, 0.088]), np.array([0.333, 0.0, 0.316, 0.0, 0.384, 0.0, 0.0]),
              np.array([0.0, -np.pi / 2, np.pi / 2, np.pi / 2, -np.pi / 2, np.pi / 2, np.pi / 2]),
              np.array([4.97, 0.647, 3.228, 3.588, 1.226, 1.667, 1.495]),
              np.array([[0.0039, 0.0021, -0.0476], [-0.0031, -0.0287, 0.0035], [0.0275, 0.0392, -0.0665],
                        [-0.0532, 0.1044, 0.0275], [-0.0118, 0.0411, -0.0384], [0.0601, -0.0141, -0.0105],
                        [0.0054, -0.0021, 0.1050]]),
              np.array([[0.70, 0.71, 0.0091], [0.0080, 0.0281, 0.0260], [0.0372, 0.0362, 0.0108], [0.0259, 0.0196, 0.0283],
                        [0.0355, 0.0295, 0.0086], [0.0020, 0.0043, 0.0054], [0.0260, 0.0240, 0.0060]]))
    rng = np.random.RandomState(5)
    lo_q = np.array([-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973])
    hi_q = np.array([2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973])
    eps = 1e-5
    for _ in range(8):
        q = rng.uniform(lo_q, hi_q)
        qd = rng.uniform(-1.5, 1.5, 7)
        M, _ = _panda_lagrangian(q, params)
        assert np.abs(lo.mass_matrix(q) - M).max() < 2e-5 * max(1.0, np.abs(M).max())
        # gravity torque = gradient of the potential energy (central differences in float64)
        g = np.array([(_panda_lagrangian(q + eps * e, params)[1] - _panda_lagrangian(q - eps * e, params)[1]) / (2 * eps)
                      for e in np.eye(7)])
        assert np.abs(lo.gravity_torque(q) - g).max() < 2e-4
        # Coriolis / centrifugal torque from the derivatives of M
        dM = [(_panda_lagrangian(q + eps * e, params)[0] - _panda_lagrangian(q - eps * e, params)[0]) / (2 * eps)
              for e in np.eye(7)]
        Mdot = sum(dM[k] * qd[k] for k in range(7))
        c = Mdot @ qd - 0.5 * np.array([qd @ dM[k] @ qd for k in range(7)])
        c_model = lo.inverse_dynamics(q, qd, np.zeros(7), gravity=0.0)
        assert np.abs(c_model - c).max() < 5e-4, (c_model, c)
        # and the full inverse dynamics is linear in the acceleration: tau(qdd) - tau(0) = M qdd
        qdd = rng.uniform(-2, 2, 7)
        tau = lo.inverse_dynamics(q, qd, qdd) - lo.inverse_dynamics(q, qd, np.zeros(7))
        assert np.abs(tau - M @ qdd).max() < 2e-4


# ---------------------------------------------------------------------------------------------- off the defaults (tests/lift_cases.py)
def test_timer_resamples_of_one_episode_draw_afresh(lo):
    """command_resampling_time = 0.3 s: the timer fires every fifteenth step, about sixteen times per episode.  Each firing draws
    at Philox counter (global id, resets so far, 1, 1 + k), k = word 63 = the firings since the env's last reset: the commands of
    one episode are pairwise distinct, lie inside the ranges, differ between envs, and each equals the value worked out by hand
    from the package's numpy Philox to 1 ulp (lift_cases.by_hand_command); the word returns to 0 at a reset.  The firings are
    found from the timer word, not from word 63."""
    import lift_cases as LC
    n, offset = 61, 5
    cfg = lo.default_config(cmd_resample_time=0.3, seed_lo=11, seed_hi=3)
    S = lo.new_state(n)
    lo.reset(cfg, S, offset)
    assert (S[:, lo.CMD_COUNT].view(np.uint32) == 0).all()
    rng = np.random.RandomState(0)
    gid = offset + np.arange(n)
    episodes = {}                                      # (env, resets so far) -> commands of the timer firings
    time_outs = 0
    for k in range(300):
        before = S[:, lo.CMD_COUNT].view(np.uint32).copy()
        _, _, term, trunc, _ = lo.step(cfg, S, LC.actions(rng, k, n), offset)
        reset = (term | trunc).astype(bool)
        fired = S[:, lo.TIME_LEFT] == np.float32(0.3)            # a resample leaves the full time; a reset's is one step short
        assert not (fired & reset).any()
        count, index = S[:, lo.RESET_COUNT].view(np.uint32), S[:, lo.CMD_COUNT].view(np.uint32)
        assert np.array_equal(index, np.where(reset, 0, before + fired)), k
        time_outs += int(trunc.sum())
        if fired.any():
            want = LC.by_hand_command(cfg, gid[fired], count[fired], index[fired])       # 1 + k, k = the index before this firing
            got = S[fired, lo.CMD:lo.CMD + 3]
            assert (np.abs(got - want) <= np.spacing(np.abs(want))).all(), k
            assert (S[fired, lo.CMD + 3:lo.CMD + 7] == np.array([1, 0, 0, 0], np.float32)).all()
            assert len(np.unique(got, axis=0)) == int(fired.sum()), "two envs drew the same command"
            for e in np.nonzero(fired)[0]:
                episodes.setdefault((int(e), int(count[e])), []).append(tuple(got[e]))
    assert time_outs == n
    firings = [len(v) for v in episodes.values()]
    # 0.3 s in steps of 0.02 s runs out after 15 or 16 steps (float32 rounding decides): 15 or 16 firings in 250 steps, 3 in the last 50
    assert len(episodes) == 2 * n and max(firings) in (15, 16) and sum(firings) >= 18 * n
    for cmds in episodes.values():
        assert len(set(cmds)) == len(cmds), "a timer resample repeated a command of its episode"
        c = np.array(cmds)
        assert (c[:, :2] >= 0.3).all() and (c[:, :2] <= 0.7).all() and (c[:, 2] == 0).all()


@pytest.mark.parametrize("n,seed", [(64, 0), (333, 5), (61, 2), (64, 3), (13, 6)])
def test_default_configuration_never_draws_on_the_timer(lo, n, seed):
    """The 300 steps of tests/test_gpu_lift.py's rollout: the time-out reset refills the timer before it runs out, so the
    resample index stays 0 and the default configuration's bits are what they were."""
    cfg = lo.default_config(seed_lo=seed)
    S = lo.new_state(n)
    lo.reset(cfg, S)
    rng = np.random.RandomState(seed)
    for k in range(300):
        a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        if k % 50 < 25:
            a[:, 7] = -1.0
        lo.step(cfg, S, a)
    assert (S[:, lo.CMD_COUNT].view(np.uint32) == 0).all() and (S[:, lo.RESET_COUNT].view(np.uint32) == 2).all()


def test_lift_cases_reach_what_the_default_never_does(lo):
    """Every case of tests/lift_cases.py on the oracle alone: finite throughout, every field of lift_config moved by some case,
    and over all cases each of drop, time-out, timer resample, timer resample in the step of a reset, a wave of eight envs with
    mixed reset lanes / mixed resample lanes, a step with both a drop and a time-out happens at least 5 times; the staggered
    case alone has at least 5 wave-steps of each mixed kind."""
    import lift_cases as LC
    assert LC.moved_fields(lo) == set(LC.CONFIG_FIELDS) == {name for name, _ in lo.Config._fields_}
    total = {}
    for case in LC.CASES:
        run = LC.case_run(lo, case)
        assert 7 <= case.n <= 37 and 40 <= case.steps <= 120
        for s in run.steps:
            assert np.isfinite(s["S"][:, :lo.RESET_COUNT]).all() and np.isfinite(s["obs"]).all() and np.isfinite(s["rew"]).all(), case.name
        counts = LC.reach_counts(run)
        print(case.name, case.n, case.steps, counts)
        for k, v in counts.items():
            total[k] = total.get(k, 0) + v
        if case.name == "stagger":
            assert counts["mixed_reset_waves"] >= 5 and counts["mixed_resample_waves"] >= 5, counts
            assert counts["drops"] >= 5 and counts["time_outs"] >= 5, counts
    print("all cases", total)
    assert all(v >= 5 for v in total.values()) and len(total) == 7, total
    by_name = {c.name: LC.reach_counts(LC.case_run(lo, c)) for c in LC.NAMED}
    assert by_name["no_sweeps"]["drops"] >= 50                                     # the cube sinks through the table
    assert by_name["reset_every_step"]["resample_with_reset"] == 11 * 40           # every env, every step
    # a resampling time of one step: once an env's staggered timer (at most 15 steps) has run out, it fires every step
    assert all(s["resampled"].all() for s in LC.case_run(lo, LC.BY_NAME["commands"]).steps[15:])


def test_lift_shards_equal_the_whole(lo):
    """RNG keyed by the global env id: reset and 40 staggered steps of 17 envs at env_id_offset = 64 equal 8 envs at 64 next
    to 9 at 72, bit for bit -- state, observations, rewards, flags."""
    import lift_cases as LC
    over = {"cmd_resample_time": 0.3, "seed_lo": 9, **LC.episode(30)}
    whole = LC.oracle_run(lo, over, 17, 40, seed=4, env_id_offset=64)
    assert LC.reach_counts(whole)["resamples"] >= 17 and LC.reach_counts(whole)["time_outs"] >= 17
    cfg = LC.oracle_config(lo, over)
    for lo_row, hi_row, offset in ((0, 8, 64), (8, 17, 72)):
        m = hi_row - lo_row
        S = lo.new_state(m)
        obs = lo.reset(cfg, S, offset)
        assert np.array_equal(obs.view(np.int32), whole.obs_reset[lo_row:hi_row].view(np.int32))
        assert np.array_equal(S.view(np.int32), whole.S_reset[lo_row:hi_row].view(np.int32))
        S[:] = whole.S0[lo_row:hi_row]
        for k, s in enumerate(whole.steps):
            obs, rew, term, trunc, _ = lo.step(cfg, S, s["a"][lo_row:hi_row], offset)
            for got, want in ((obs, s["obs"]), (rew, s["rew"]), (S, s["S"])):
                assert np.array_equal(got.view(np.int32), want[lo_row:hi_row].view(np.int32)), (offset, k)
            assert np.array_equal(term.astype(bool), s["term"][lo_row:hi_row]) and np.array_equal(trunc.astype(bool), s["trunc"][lo_row:hi_row])
