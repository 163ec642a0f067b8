#!/usr/bin/env python3
"""Dev tool (build container): are the functions of two hipcc -S listings the same machine code?  For a refactor that moves
source text between files and must not move a kernel.

    hipcc <build.FLAGS> --cuda-device-only -S -o old/td3_kernels.s isaac_rover_orbit_amd/csrc/td3_kernels.hip    # at the parent
    hipcc <build.FLAGS> --cuda-device-only -S -o new/td3_kernels.s isaac_rover_orbit_amd/csrc/td3_kernels.hip    # at the head
    python tools/isa_same.py old/td3_kernels.s new/td3_kernels.s

Per function one line: its base name, the instruction count and sha256[:12] of the first listing's stream, the kernel
descriptor's register / LDS / scratch values, and SAME or DIFFERENT (then with the second listing's figures).  Compared are
the instruction lines (comments stripped, directives dropped, local label numbers and symbol names normalised) and
.amdhsa_next_free_vgpr, .amdhsa_next_free_sgpr, .amdhsa_accum_offset, .amdhsa_group_segment_fixed_size and
.amdhsa_private_segment_fixed_size.  Functions are paired by base name: the td3_ / sac_ / offpolicy_ / ppo_ / lift_ / dagger_ /
dagger_conv_ prefix (also as rover_td3_collect_ / rover_sac_collect_ / offpolicy_collect_) and template arguments are ignored, several functions of one base
name (a template's instantiations) pair in their order of appearance.
A function only one listing has is reported and fails the comparison, unless --common is given (two different files that share
some kernels: python tools/isa_same.py --common new/td3_kernels.s new/sac_kernels.s, or new/ppo_kernels.s new/lift_ppo_kernels.s).
Exit status 0: everything compared is SAME.

The tool only diffs text; it knows nothing about particular instructions."""
import hashlib
import re
import sys

DESC = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")
SYMBOL = re.compile(r"\b_Z\w+")


def base_name(sym):
    """The source identifier of an Itanium-mangled function name (the last one of a nested name), without the trainer prefix."""
    name = sym
    if sym.startswith("_Z"):
        i, ids = (3 if sym.startswith("_ZN") else 2), []
        i += sym[i:i + 1] == "L"                                               # internal linkage
        while i < len(sym) and sym[i].isdigit():
            j = i
            while sym[j].isdigit():
                j += 1
            n = int(sym[i:j])
            ids.append(sym[j:j + n])
            i = j + n
        if ids:
            name = ids[-1]
    return re.sub(r"^(dagger_conv|dagger|rover_(td3|sac)_collect|offpolicy_collect|td3|sac|offpolicy|ppo|lift)_", "", name)


def normalise(line):
    line = line.split(";")[0].strip()
    line = re.sub(r"\.L([A-Za-z_]+?)\d+_(\d+)", r".L\1_\2", line)              # .LBB<function number>_<block>
    return SYMBOL.sub(lambda m: base_name(m.group(0)), line)


def functions(path):
    """[(base name, [instruction and label lines], {descriptor values})] in the listing's order."""
    out, cur, desc_of = [], None, {}
    kernel = None
    for raw in open(path):
        s = raw.strip()
        m = re.match(r"\.type\s+(\S+),@function", s)
        if m:
            cur = [m.group(1), None]
            continue
        if cur and cur[1] is None:
            if s.split(";")[0].strip() == cur[0] + ":":
                cur[1] = []
                out.append(cur)
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            kernel = desc_of.setdefault(m.group(1), {})
            continue
        if s == ".end_amdhsa_kernel":
            kernel = None
            continue
        if kernel is not None:
            m = re.match(r"\.amdhsa_(\w+)\s+(.*)", s)
            if m and m.group(1) in DESC:
                kernel[m.group(1)] = m.group(2).strip()
            continue
        if cur:
            if s.startswith((".section", ".Lfunc_end")):
                cur = None
                continue
            t = normalise(s)
            if not t or (t.startswith(".") and not t.endswith(":")):
                continue
            cur[1].append(t)
    return [(base_name(sym), body, desc_of.get(sym, {})) for sym, body in out]


def figures(body, desc):
    n = sum(1 for t in body if not t.endswith(":"))
    h = hashlib.sha256("\n".join(body).encode()).hexdigest()[:12]
    d = " ".join(f"{k.split('_fixed')[0].replace('next_free_', '')}={desc[k]}" for k in DESC if k in desc)
    return f"{n:5d} instr  {h}  {d}".rstrip()


def main():
    args = [a for a in sys.argv[1:] if a != "--common"]
    common = "--common" in sys.argv[1:]
    if len(args) != 2:
        sys.exit(__doc__)
    a, b = functions(args[0]), functions(args[1])
    pool, bad = {}, 0
    for name, body, desc in b:
        pool.setdefault(name, []).append((body, desc))
    for name, body, desc in a:
        if not pool.get(name):
            if not common:
                bad += 1
                print(f"{name:34s} {figures(body, desc)}  ONLY IN {args[0]}")
            continue
        body_b, desc_b = pool[name].pop(0)
        if body == body_b and desc == desc_b:
            print(f"{name:34s} {figures(body, desc)}  SAME")
        else:
            bad += 1
            print(f"{name:34s} {figures(body, desc)}  DIFFERENT: {figures(body_b, desc_b)}")
    if not common:
        for name, rest in pool.items():
            for body, desc in rest:
                bad += 1
                print(f"{name:34s} {figures(body, desc)}  ONLY IN {args[1]}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
