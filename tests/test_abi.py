"""The C-ABI library loads on a CPU-only host and exports every symbol include/*.h declares; model constants
agree between the HIP library, the oracle and the fixture derived from the reference asset.  No compute calls."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


DEBUG_HEADER = "rover_debug.h"      # test-only / measurement-only hooks: declared, exported, not part of the boundary


def declared_symbols(debug=False):
    names = set()
    for hdr in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if hdr.endswith(".h") and (hdr == DEBUG_HEADER) == debug:
            src = open(os.path.join(ROOT, "include", hdr)).read()
            src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
            names |= set(re.findall(r"\b(rover_[a-z0-9_]+)\s*\(", src))
    return sorted(names)


def test_library_exports_every_declared_symbol():
    from isaac_rover_orbit_amd import _lib, build
    build.build_extension()
    lib = _lib.load()
    names = declared_symbols()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/*.h but not exported"
    assert sorted(_lib.EXPORTS) == names, "python binding and header disagree on the entry points"
    # ... and the converse: the library exports NOTHING that no header declares -- the boundary headers plus the
    # hooks of include/rover_debug.h (marked test-only there)
    import subprocess
    debug = declared_symbols(debug=True)
    assert debug == ["rover_debug_set_fused", "rover_lift_debug_set_lanes", "rover_lift_debug_set_pipeline"]
    for n in debug:
        assert hasattr(lib, n), f"{n} declared in include/{DEBUG_HEADER} but not exported"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in nm.splitlines() if len(l.split()) == 3 and l.split()[1] in "TW" and l.split()[-1].startswith("rover_"))
    assert exported == sorted(names + debug), sorted(set(exported) ^ set(names + debug))
    assert lib.rover_config_bytes() == C.sizeof(_lib.RoverConfig)
    assert lib.rover_state_words() == 72
    assert b"gfx950" in lib.rover_version()


def test_code_object_is_gfx950():
    from isaac_rover_orbit_amd import _lib
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in data and b"rover_step_kernel" in data and b"rover_scan_obs_kernel" in data


def test_default_config_matches_reference_cfg_and_oracle(oracle):
    from isaac_rover_orbit_amd import _lib
    c, o = _lib.default_config(), oracle.default_config()
    for name, _ in _lib.RoverConfig._fields_:
        a, b = getattr(c, name), getattr(o, name)
        if name == "rew_weight":
            assert list(a) == list(b) == pytest.approx([5.0, 5.0, -0.1, -1.5, -0.5, -2.0, -2.0])
        else:
            assert a == b, name
    assert c.decimation == 6 and c.max_episode_length == 750 and c.scan_nx == 31 and c.scan_ny == 31
    assert c.offset_lin == c.offset_ang == pytest.approx(-0.0135)


def test_lift_model_constants_agree_and_step_kernel_has_no_scratch():
    """FrankaCubeLift-v0: the HIP library and the separately written oracle carry the same model constants; the step
    kernel keeps everything in registers (no private segment = no scratch memory) and uses 2176 B of LDS (the lane exchange)."""
    import subprocess
    from isaac_rover_orbit_amd import _lib
    from oracle import lift_oracle as lo
    lib = _lib.load()
    n = lib.rover_lift_model_constants(None, 0)
    hip = np.zeros(n, np.float32)
    lib.rover_lift_model_constants(hip.ctypes.data_as(C.c_void_p), n)
    orc = lo.model_constants()
    assert n == len(orc) > 100 and np.array_equal(hip, orc)
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("ROCm llvm tools not installed")
    import tempfile
    from helpers import gfx950_code_objects
    found = 0
    for blob in gfx950_code_objects(_lib.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob)
            f.flush()
            notes = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True).stdout
        # one YAML map per kernel: split at the '- .agpr_count' / '- .args' list heads
        for entry in re.split(r"\n\s*- \.", notes):
            m = re.search(r"\.name:\s*(\S*lift_step_kernel\S*)", entry)
            if not m or ".private_segment_fixed_size" not in entry:
                continue
            found += 1
            assert re.search(r"\.private_segment_fixed_size:\s*0\b", entry), f"{m.group(1)} uses scratch memory"
            # one 2176-byte exchange slot set per wave; the two-wave pipelined form adds its hand-off buffers: 6144 bytes
            assert re.search(r"\.group_segment_fixed_size:\s*(2176|6144)\b", entry), f"{m.group(1)}: unexpected LDS size"
    assert found >= 3, "lift_step_kernel<8, true> / <8, false> / <16, false> not found in the code object metadata"
    # the rover step kernels at one wave per SIMD: no scratch either, no static LDS (a promoted alloca would make the kernel read
    # its workgroup size from the dispatch packet in host memory: DESIGN 3.1), and the one-launch form is a 512-thread workgroup
    seen = {}
    for blob in gfx950_code_objects(_lib.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob)
            f.flush()
            notes = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True).stdout
        for entry in re.split(r"\n\s*- \.", notes):
            m = re.search(r"\.name:\s*(\S*(rover_step_kernel_group|rover_step_scan_kernel)\S*)", entry)
            if not m or ".private_segment_fixed_size" not in entry:
                continue
            seen[m.group(2)] = seen.get(m.group(2), 0) + 1
            assert re.search(r"\.private_segment_fixed_size:\s*0\b", entry), f"{m.group(1)} uses scratch memory"
            assert re.search(r"\.group_segment_fixed_size:\s*0\b", entry), f"{m.group(1)}: static LDS"
            if m.group(2) == "rover_step_scan_kernel":
                assert re.search(r"\.max_flat_workgroup_size:\s*512\b", entry), f"{m.group(1)}: four step waves + four copy waves"
    assert seen.get("rover_step_kernel_group", 0) >= 1 and seen.get("rover_step_scan_kernel", 0) >= 2, seen


def test_errors_are_codes_not_crashes():
    """Error behaviour of the boundary: int codes + rover_last_error(), also on a host without a GPU."""
    from isaac_rover_orbit_amd import _lib
    lib = _lib.load()
    assert lib.rover_default_config(None) == 1
    assert b"NULL" in lib.rover_last_error()
    cfg = _lib.default_config()
    h = C.c_void_p()
    assert lib.rover_create(C.byref(cfg), 0, 0, 0, C.byref(h)) == 1           # num_envs must be > 0
    bad = _lib.default_config()
    bad.scan_nx = 0
    assert lib.rover_create(C.byref(bad), 16, 0, 0, C.byref(h)) == 1
    assert lib.rover_step(None, None, None, None, None, None, None, None, None) == 1
    assert lib.rover_workspace_bytes(None) == 0
    import torch
    if not torch.cuda.is_available():
        rc = lib.rover_create(C.byref(cfg), 16, 0, 0, C.byref(h))
        assert rc == 3 and len(lib.rover_last_error()) > 0                    # ROVER_ERR_HIP, no device
        with pytest.raises(_lib.RoverHipError):
            from isaac_rover_orbit_amd.envs import RoverEnv
            RoverEnv()                                                         # product path fails loudly, no CPU fallback


def test_model_constants_agree(oracle):
    from isaac_rover_orbit_amd import _lib
    lib = _lib.load()
    n = lib.rover_model_constants(None, 0)
    hip = np.zeros(n, np.float32)
    lib.rover_model_constants(hip.ctypes.data_as(C.c_void_p), n)
    orc = oracle.model_constants()
    assert n == len(orc) and np.array_equal(hip, orc)
    j = json.load(open(os.path.join(ROOT, "tests", "golden", "rover_model.json")))
    assert hip[0] == j["total_mass"] == 25.0
    assert np.allclose(hip[1:4], j["com"], atol=1e-6) and np.allclose(hip[4:7], j["inertia_diag"], atol=1e-6)
    wheels = np.array([j["wheel_centres"][k] for k in ["FL", "FR", "CL", "CR", "RL", "RR"]]).ravel()
    assert np.allclose(hip[7:25], wheels, atol=1e-6)
    bog = ["FL_Boogie", "FR_Boogie", "R_Boogie"]
    assert np.allclose(hip[25:34], np.array([j["bogies"][b]["pivot"] for b in bog]).ravel(), atol=1e-6)
    assert np.allclose(hip[34:43], np.array([j["bogies"][b]["axis"] for b in bog]).ravel(), atol=1e-6)
    assert np.allclose(hip[43:46], [j["bogies"][b]["inertia"] for b in bog], atol=1e-6)
    assert abs(hip[46] - j["wheel_contact_radius"]) < 1e-6
    # actuator values of aau_rover_simple.py:42-64
    assert list(hip[48:52]) == [8000.0, 1000.0, 12.0, 6.0] and list(hip[53:57]) == [100.0, 4000.0, 12.0, 6.0]
