"""tools/isa_same.py on synthetic listings: the name pairing (trainer prefixes old and new, template instantiations), the
normalisation of labels and symbols, and both verdicts.  No compiler and no GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_same  # noqa: E402

PPO_SUMSQ = "_ZN12_GLOBAL__N_116ppo_sumsq_kernelEPKfiPf"
LIFT_SUMSQ = "_ZN12_GLOBAL__N_117lift_sumsq_kernelEPKfiPfPK20rover_lift_ppo_state"
TD3_DENSE = "_ZN12_GLOBAL__N_122offpolicy_dense_kernelI14rover_td3_stateEEvNS_11DenseLaunchE"
SAC_DENSE = "_ZN12_GLOBAL__N_122offpolicy_dense_kernelI14rover_sac_stateEEvNS_11DenseLaunchE"


@pytest.mark.parametrize("symbol, base", [
    ("_ZN12_GLOBAL__N_117td3_smooth_kernelEPfPKfifff", "smooth_kernel"),               # the old prefixes
    ("_ZN12_GLOBAL__N_119sac_min_head_kernelEPKfS1_Pfi", "min_head_kernel"),
    (TD3_DENSE, "dense_kernel"),                                                       # ... under a template argument
    ("_Z28rover_td3_collect_act_kernelPKfi", "act_kernel"),
    ("_Z28rover_sac_collect_act_kernelPKfi", "act_kernel"),
    ("_ZN12_GLOBAL__N_131offpolicy_collect_record_kernelILb1ENS_9RecLaunchEEEvT0_", "record_kernel"),
    (PPO_SUMSQ, "sumsq_kernel"),                                                       # the on-policy prefixes
    (LIFT_SUMSQ, "sumsq_kernel"),
    ("_ZN12_GLOBAL__N_116ppo_wgrad_kernelINS_9WgradArgsEEEvT_", "wgrad_kernel"),       # a template instantiation
    ("_ZN12_GLOBAL__N_116ppo_wgrad_kernelINS_14WgradArgsGatedEEEvT_", "wgrad_kernel"),
    ("_ZN12_GLOBAL__N_116trpo_adam_kernelEPfS0_S0_S0_PK16rover_trpo_stateifffS0_i", "trpo_adam_kernel"),   # no prefix of the list
    ("lift_rollout_act_kernel", "rollout_act_kernel"),                                 # unmangled
    ("_ZN12_GLOBAL__N_12LKE", "LK"),                                                   # a table
])
def test_base_name(symbol, base):
    assert isa_same.base_name(symbol) == base


def test_normalise():
    # a comment goes, the function's number leaves its block labels, a symbol becomes its base name
    assert isa_same.normalise("\ts_cbranch_scc1 .LBB12_3 ; encoding") == "s_cbranch_scc1 .LBB_3"
    assert isa_same.normalise(".LBB7_10:") == ".LBB_10:"
    assert (isa_same.normalise(f"s_add_u32 s2, s2, {PPO_SUMSQ}@rel32@lo+4")
            == isa_same.normalise(f"s_add_u32 s2, s2, {LIFT_SUMSQ}@rel32@lo+4")
            == "s_add_u32 s2, s2, sumsq_kernel@rel32@lo+4")
    assert isa_same.normalise("; only a comment") == ""


def listing(number, symbol, instructions, vgpr=7):
    """One kernel as hipcc -S lays it out: the function, then its descriptor."""
    body = "\n".join(f"\t{i}" for i in instructions)
    return (f"\t.text\n\t.type\t{symbol},@function\n{symbol}:                      ; @{symbol}\n; %bb.0:\n{body}\n"
            f".Lfunc_end{number}:\n\t.size\t{symbol}, .Lfunc_end{number}-{symbol}\n\t.section\t.rodata,\"a\",@progbits\n"
            f"\t.amdhsa_kernel {symbol}\n\t\t.amdhsa_group_segment_fixed_size 1024\n\t\t.amdhsa_private_segment_fixed_size 0\n"
            f"\t\t.amdhsa_next_free_vgpr {vgpr}\n\t\t.amdhsa_next_free_sgpr 12\n\t\t.amdhsa_accum_offset 8\n\t.end_amdhsa_kernel\n\t.text\n")


def three(fn):
    return [f"s_load_dword s2, s[0:1], 0x0 ; {fn}", f"s_cbranch_scc1 .LBB{fn}_1", "s_endpgm"]


def run(tmp_path, capsys, a, b, *flags):
    pa, pb = tmp_path / "a.s", tmp_path / "b.s"
    pa.write_text(a)
    pb.write_text(b)
    argv, sys.argv = sys.argv, ["isa_same.py", *flags, str(pa), str(pb)]
    try:
        with pytest.raises(SystemExit) as stop:
            isa_same.main()
    finally:
        sys.argv = argv
    return stop.value.code, capsys.readouterr().out.splitlines()


def test_same_across_prefixes_and_function_numbers(tmp_path, capsys):
    # ppo_sumsq_kernel as function 3 of one listing against lift_sumsq_kernel as function 5 of the other; a template's two
    # instantiations pair in their order of appearance
    a = listing(3, PPO_SUMSQ, three(3)) + listing(4, TD3_DENSE, three(4)) + listing(5, SAC_DENSE, three(5), vgpr=9)
    b = listing(5, LIFT_SUMSQ, three(5)) + listing(6, SAC_DENSE, three(6)) + listing(7, TD3_DENSE, three(7), vgpr=9)
    code, out = run(tmp_path, capsys, a, b)
    assert code == 0
    assert [line.split()[0] for line in out] == ["sumsq_kernel", "dense_kernel", "dense_kernel"]
    assert all(line.endswith("SAME") and "    3 instr" in line for line in out)
    assert "vgpr=7 sgpr=12 accum_offset=8 group_segment=1024 private_segment=0" in out[0]


def test_different_stream_descriptor_and_missing_function(tmp_path, capsys):
    moved = ["s_load_dword s2, s[0:1], 0x0", "s_cbranch_scc0 .LBB5_1", "s_endpgm"]              # one branch inverted
    a = listing(3, PPO_SUMSQ, three(3))
    code, out = run(tmp_path, capsys, a, listing(5, LIFT_SUMSQ, moved))
    assert code == 1 and len(out) == 1 and "DIFFERENT:" in out[0]
    code, out = run(tmp_path, capsys, a, listing(5, LIFT_SUMSQ, three(5), vgpr=8))              # the stream is the same, a register more
    assert code == 1 and "DIFFERENT:" in out[0] and "vgpr=8" in out[0].split("DIFFERENT:")[1]
    both = a + listing(4, TD3_DENSE, three(4))
    code, out = run(tmp_path, capsys, both, listing(5, LIFT_SUMSQ, three(5)))                   # dense_kernel in one listing only
    assert code == 1 and out[0].endswith("SAME") and "ONLY IN" in out[1]
    code, out = run(tmp_path, capsys, both, listing(5, LIFT_SUMSQ, three(5)), "--common")
    assert code == 0 and len(out) == 1 and out[0].endswith("SAME")
