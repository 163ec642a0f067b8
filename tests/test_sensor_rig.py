"""The sensor rig's schedule (``envs/_sensors.py``) on the CPU: a rig built on ``device="cpu"`` over recording
stand-ins for the render, the sensor model, the depth noise, the lidar's cast and noise and the map.  Every stand-in writes a
value made of its stage and its call number into the buffer it is handed and logs its arguments; the test drives the rig as the
env does (reset, seven steps, a reset with draws on a mask, two steps) and checks which stage ran when, with which counter,
into which buffer, and what ``extras`` holds afterwards."""
import inspect

import pytest
import torch

from isaac_rover_orbit_amd.envs import _sensors, rover_env
from isaac_rover_orbit_amd.envs._sensors import KEYS, SensorRig

N, H, W, CH, AZ, COLS = 3, 4, 2, 2, 3, 5
CAMERA_EVERY, LIDAR_EVERY = 3, 2
MAP_KEYS = ("elevation_scan", "elevation_known", "elevation_count")


class Stage:
    """``apply`` of the sensor model / the noise stages: adds ``step`` to the buffer, so the image tells which stages it passed."""

    def __init__(self, log, name, step):
        self.log, self.name, self.step, self.calls, self.seed = log, name, step, 0, 7

    def apply(self, buf, counter, **kw):
        self.calls += 1
        buf.add_(self.step)
        if kw.get("valid_out") is not None:
            kw["valid_out"].fill_(self.calls)
        self.log.append((self.name, {"buf": buf, "counter": counter, **kw}))


class LidarStandIn:
    channels, azimuths, rays = CH, AZ, CH * AZ

    def __init__(self, log):
        self.log, self.calls = log, 0

    def cast(self, buf, hits):
        self.calls += 1
        buf.fill_(100 + self.calls)
        if hits is not None:
            hits.fill_(200 + self.calls)
        self.log.append(("cast", {"buf": buf, "hits": hits}))


class MapStandIn:
    columns = COLS

    def __init__(self, log):
        self.log, self.calls = log, 0

    def update(self, depth, pos, quat, reset=(None, None), scan_out=None, known_out=None, count_out=None):
        self.calls += 1
        scan_out.fill_(300 + self.calls), known_out.fill_(self.calls), count_out.fill_(self.calls)
        self.log.append(("map", {"depth": depth, "pos": pos, "quat": quat, "reset": reset, "outs": (scan_out, known_out, count_out)}))

    def clear(self):
        self.log.append(("clear", {}))

    def state_dict(self):
        return {"elevation_map": torch.full((N, 2, 2), float(self.calls)), "elevation_origin": torch.zeros(N, 2)}

    def load_state_dict(self, sd):
        self.log.append(("load", {"sd": sd}))


class Host:
    """What the rig reads of the env: ``extras`` and the two counters, advanced as the env advances them."""

    def __init__(self):
        self.extras, self.common_step_counter, self.call_counter = {"log": {}}, 0, 0


def build(camera, lidar, source, bare=False):
    host, log = Host(), []
    renders = []

    def render(cfg, ws, buf):
        assert cfg == "camera-cfg" and ws == "workspace"
        renders.append(buf)
        buf.fill_(len(renders))
        log.append(("render", {"buf": buf}))

    kw = {"pose": (torch.zeros(N, 3), torch.zeros(N, 4))}
    if camera:
        kw.update(render=render, camera_cfg="camera-cfg", workspace="workspace", image=(H, W), camera_every=CAMERA_EVERY)
        if not bare:
            kw.update(depth_sensor=Stage(log, "sensor", 0.25), depth_post=Stage(log, "post", 0.5))
    if lidar:
        kw.update(lidar=LidarStandIn(log), lidar_hits=not bare, lidar_every=LIDAR_EVERY)
        if not bare:
            kw.update(lidar_post=Stage(log, "lidar_post", 0.5))
    if source is not None:
        kw.update(elevation=MapStandIn(log), map_source=source, unknown_value=-1.0)
    return host, log, SensorRig(host, "cpu", N, **kw), kw


def expected_stages(camera, lidar, source, bare, force, step):
    """The schedule as the issue states it: (names in order, lidar frame?, camera frame?)."""
    names = []
    lidar_frame = lidar and (force or step % LIDAR_EVERY == 0)
    camera_frame = camera and (force or step % CAMERA_EVERY == 0)
    if lidar_frame:
        names += ["cast"] if bare else ["cast", "lidar_post"]
    if lidar and source == "lidar":
        names += ["map"]
    if camera_frame:
        names += ["render"] if bare else ["render", "sensor", "post"]
    if camera and source == "camera":
        names += ["map"]
    return names, lidar_frame, camera_frame


CONFIGS = {"camera": (True, False, None, False), "lidar": (False, True, None, False), "camera+lidar": (True, True, None, False),
           "bare camera+lidar": (True, True, None, True), "camera+map+lidar": (True, True, "camera", False),
           "lidar+map": (False, True, "lidar", False), "camera+lidar+map": (True, True, "lidar", False)}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_the_schedule_runs_each_stage_when_with_which_counter_into_which_buffer(name):
    camera, lidar, source, bare = CONFIGS[name]
    host, log, rig, parts = build(camera, lidar, source, bare)
    has_map = source is not None
    assert rig.active and (not camera or rig.camera_every == CAMERA_EVERY) and (not lidar or rig.lidar_every == LIDAR_EVERY)
    keys = set()
    if camera:
        keys |= {"depth", "rgb"} | (set() if bare else {"depth_valid"})
    if lidar:
        keys |= {"lidar_range"} | (set() if bare else {"lidar_hits_w"})
    if has_map:
        keys |= set(MAP_KEYS)
    assert set(host.extras) == keys | {"log"} and (not camera or host.extras["rgb"] is None)
    if camera:
        assert host.extras["depth"].shape == (N, W, H) and bool(torch.isinf(host.extras["depth"]).all())
    if has_map:
        assert bool((host.extras["elevation_scan"] == -1.0).all()) and host.extras["elevation_scan"].shape == (N, COLS)

    history = {k: [] for k in KEYS}                    # per key: (tensor, copy) of every frame published
    mask = torch.tensor([0, 1, 0], dtype=torch.uint8)
    calls = ["reset"] + ["step"] * 7 + ["draws"] + ["step"] * 2
    maps = 0
    for kind in calls:
        del log[:]
        host.call_counter += 1                         # one launch left the state ...
        flags = (None, None)
        if kind == "reset":
            rig.clear()
            rig.update(force=True)
        elif kind == "step":
            host.common_step_counter += 1
            flags = (torch.zeros(N, dtype=torch.uint8), torch.zeros(N, dtype=torch.uint8))
            rig.update(reset=flags)
        else:
            rig.update_after_draws(mask)
        counter = max(host.call_counter - 1, 0)        # ... and its counter keys every draw of the frames of that state
        force = kind != "step"
        names, lidar_frame, camera_frame = expected_stages(camera, lidar, source, bare, force, host.common_step_counter)
        if kind == "reset" and has_map:
            names = ["clear"] + names
        if kind == "draws" and not has_map:            # the lidar alone takes a frame; a camera alone takes none
            names, camera_frame = [n for n in names if n in ("cast", "lidar_post")], False
        assert [n for n, _ in log] == names, (kind, host.common_step_counter)
        got = dict(log)
        assert all(a["counter"] == counter for _, a in log if "counter" in a)
        ex = host.extras
        assert set(ex) == keys | {"log"}
        if lidar_frame:
            k = parts["lidar"].calls
            assert got["cast"]["buf"] is ex["lidar_range"] and ex["lidar_range"].shape == (N, CH, AZ)
            assert bool((ex["lidar_range"] == 100 + k + (0.0 if bare else 0.5)).all())
            if bare:
                assert got["cast"]["hits"] is None
            else:
                assert got["cast"]["hits"] is ex["lidar_hits_w"] and bool((ex["lidar_hits_w"] == 200 + k).all())
                assert ex["lidar_hits_w"].shape == (N, CH * AZ, 3) and got["lidar_post"]["buf"] is got["cast"]["buf"]
        if camera_frame:
            buf = got["render"]["buf"]
            assert buf.shape == (N, H, W) and buf.is_contiguous() and buf.data_ptr() == ex["depth"].data_ptr()
            assert torch.equal(ex["depth"], buf.permute(0, 2, 1))
            k = len([b for b in history["depth"]]) + 1
            assert bool((buf == k + (0.0 if bare else 0.75)).all())
            if not bare:
                assert got["sensor"]["buf"] is buf and got["post"]["buf"] is buf and got["sensor"]["valid_out"] is ex["depth_valid"]
                assert "valid_out" not in got["post"] and bool((ex["depth_valid"] == k).all()) and ex["depth_valid"].dtype == torch.int32
        if has_map:                                    # on every call, with None exactly where its sensor made no frame
            maps += 1
            a = got["map"]
            assert parts["elevation"].calls == maps and a["pos"] is parts["pose"][0] and a["quat"] is parts["pose"][1]
            frame = (got["cast"]["buf"] if lidar_frame else None) if source == "lidar" else (got["render"]["buf"] if camera_frame else None)
            assert a["depth"] is frame
            if kind == "step":
                assert a["reset"][0] is flags[0] and a["reset"][1] is flags[1]
            elif kind == "reset":
                assert tuple(a["reset"]) == (None, None)
            else:
                assert torch.equal(a["reset"][0], mask) and a["reset"][0] is not mask and a["reset"][1] is None
            assert all(o is ex[key] for o, key in zip(a["outs"], MAP_KEYS))
            assert bool((ex["elevation_scan"] == 300 + maps).all()) and bool((ex["elevation_count"] == maps).all())
        # the two-set rotation: a frame's tensors are bit-unchanged after the next frame and overwritten by the one after it
        fresh = ({"lidar_range", "lidar_hits_w"} if lidar_frame else set()) | ({"depth", "depth_valid"} if camera_frame else set())
        fresh |= set(MAP_KEYS) if has_map else set()
        for key in keys - {"rgb"}:
            h = history[key]
            if key in fresh:
                h.append((ex[key], ex[key].clone()))
                if len(h) >= 2:
                    assert h[-2][0] is not h[-1][0] and h[-2][0].data_ptr() != h[-1][0].data_ptr() and torch.equal(*h[-2])
                if len(h) >= 3:
                    assert h[-3][0].data_ptr() == h[-1][0].data_ptr() and not torch.equal(*h[-3])
            else:                                      # no frame: what is published stays, untouched
                assert h and ex[key] is h[-1][0] and torch.equal(*h[-1])
    if camera:
        assert len(history["depth"]) == (5 if has_map else 4)          # reset, steps 3, 6, (draws,) 9
    if lidar:
        assert len(history["lidar_range"]) == 6                        # reset, steps 2, 4, 6, draws, 8

    # reseed reaches the stages that have a seed, and nothing else
    rig.reseed(123)
    seeded = [parts[k] for k in ("depth_sensor", "depth_post", "lidar_post") if k in parts]
    assert all(s.seed == 123 for s in seeded) and len(seeded) == (0 if bare else 2 * camera + lidar)
    assert not any(hasattr(parts[k], "seed") for k in ("lidar", "elevation") if k in parts)
    # the checkpoint is the map's, or nothing
    if has_map:
        sd = rig.state_dict()
        assert set(sd) == {"elevation_map", "elevation_origin"} and bool((sd["elevation_map"] == maps).all())
        del log[:]
        rig.load_state_dict({"state": 0})
        assert not log
        rig.load_state_dict(sd)
        assert [n for n, _ in log] == ["load"] and log[0][1]["sd"] is sd
    else:
        assert rig.state_dict() == {} and rig.load_state_dict({"elevation_map": 0}) is None
    # a rig without sensors in its place removes every key this one published
    host.extras["mine"] = 1
    inert = SensorRig(host)
    assert set(host.extras) == {"log", "mine"} and not inert.active and inert.state_dict() == {}
    inert.clear(), inert.reseed(5), inert.update(force=True), inert.update_after_draws(None)
    assert set(host.extras) == {"log", "mine"}
    with pytest.raises(RuntimeError, match="render_depth needs a camera"):
        inert.render_depth()
    with pytest.raises(RuntimeError, match="cast_lidar needs a lidar"):
        inert.cast_lidar()


def test_fresh_frames_go_through_the_same_stages_into_new_buffers():
    host, log, rig, parts = build(True, True, None)
    host.call_counter = 5
    depth, rng = rig.render_depth(), rig.cast_lidar()
    assert [n for n, _ in log] == ["render", "sensor", "post", "cast", "lidar_post"]
    assert all(a["counter"] == 4 for _, a in log if "counter" in a) and log[1][1]["valid_out"] is None and log[3][1]["hits"] is None
    assert depth.shape == (N, W, H) and bool((depth == 1.75).all()) and depth.data_ptr() == log[0][1]["buf"].data_ptr()
    assert rng.shape == (N, CH, AZ) and bool((rng == 101.5).all())
    assert bool(torch.isinf(host.extras["depth"]).all()) and bool(torch.isinf(host.extras["lidar_range"]).all())
    rig.depth_sensor = rig.depth_post = rig.lidar_post = None          # a bench switches stages off by assignment
    del log[:]
    buf, valid = torch.zeros(N, H, W), torch.zeros(N, dtype=torch.int32)
    rig.render_into(buf, valid), rig.cast_into(torch.zeros(N, CH, AZ))
    assert [n for n, _ in log] == ["render", "cast"] and bool((buf == 2.0).all()) and not bool(valid.any())
    counts = host.extras["depth_valid"]                                # no sensor model any more: its counts are not published again
    rig.update(force=True)
    assert host.extras["depth_valid"] is counts and host.extras["depth"].data_ptr() == log[-1][1]["buf"].data_ptr()
    assert [n for n, _ in log][2:] == ["cast", "render"] and not bool(counts.any())


def test_the_step_paths_share_one_tail_and_the_env_holds_no_sensor_code():
    """``step``, ``profile_step`` and the slow path end in ``_step_counted`` / ``_step_tail``, which alone do the bookkeeping and
    call the rig behind one attribute test; what moved to ``envs/_sensors.py`` is no longer defined (or aliased) on the env."""
    env = rover_env.RoverEnv
    for path in (env.step, env.profile_step, env._step_with_user_terms):
        src = inspect.getsource(path)
        assert src.count("self._step_counted(k)") == 1 and src.count("self._step_tail(k)") == 1
        assert src.index("self._step_counted(k)") < src.index("self._step_tail(k)")
        for word in ("_bump_counter", "common_step_counter", "_log_host_stale", "_post_observations", "sensors", "_obs_dicts"):
            assert word not in src, (path.__name__, word)
    slow = inspect.getsource(env._step_with_user_terms)
    assert slow.index("_step_counted(k)") < slow.index("t.func(self") < slow.index("_lib.rover_step_finish(") < slow.index("_step_tail(k)")
    assert slow.index("_step_tail(k)") < slow.index("self._log_pending = False")
    tail = inspect.getsource(env._step_tail)
    assert "if self.sensors.active:\n            self.sensors.update(reset=(self._term[k], self._trunc[k]))" in tail
    source = inspect.getsource(rover_env)
    moved = ("_init_camera", "_init_lidar", "_init_elevation", "_camera_update", "_lidar_update", "_elevation_update", "_render_into",
             "_cast_into", "_camera_ws", "_camera_cfg", "_camera_every", "_lidar_every", "_depth_post", "_depth_sensor", "_depth_valid",
             "_depth_cur", "_lidar_post", "_lidar_range", "_lidar_hits", "_lidar_cur", "_elev_out", "_elev_mask", "_elev_pose",
             "_elev_cur", "_elev_from_lidar", "_elevation", "rover_camera_render", "rover_camera_prepare")
    for word in moved:
        assert word not in source and not hasattr(env, word), word
    assert "self._lidar" not in source and "self._depth" not in source and not hasattr(env, "_lidar")
    bare = object.__new__(env)                         # nor does an instance serve them from its rig: no forwarding on attribute look-up
    bare.__dict__["sensors"] = SensorRig(Host())
    for word in moved + ("_lidar", "_depth"):
        with pytest.raises(AttributeError):
            getattr(bare, word)
    assert env.render_depth.__doc__ and env.cast_lidar.__doc__ and "SensorRig.for_env(self)" in inspect.getsource(env.__init__)
    assert hasattr(_sensors.SensorRig, "render_into") and hasattr(_sensors.SensorRig, "cast_into")
