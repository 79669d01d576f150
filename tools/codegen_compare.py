#!/usr/bin/env python3
"""tools/codegen_compare.py <dir of tree A> <dir of tree B> [<source stem> [<kernel-name pattern>]] - kernel instantiations of one source file in
two trees, function by function: the instruction streams (comments dropped, local labels renumbered) and the compiler's resource remarks.
<source stem> defaults to k_physics and <kernel-name pattern> (a regular expression over the kernels' unqualified names) to env_kernel; e.g.
`k_fused 'fused_mlp_kernel|bf16_rowpass_kernel|gather_rows_kernel'` compares the row-pass kernels (with that file's build flags, -ffp-contract=fast,
in the command below).  Each directory holds `<source stem>.s` and `remarks.txt` of one tree:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -I<tree>/minppo_amd/csrc -I<tree>/include -Rpass-analysis=kernel-resource-usage \\
          --cuda-device-only -S <tree>/minppo_amd/csrc/k_physics.hip -o <dir>/k_physics.s 2> <dir>/remarks.txt

(cross-compiles: no GPU needed).  Kernels are matched by name; where tree B's specialised kernels carry one template argument more than tree A's (16 -> 17:
the number of ball joints in front of cparam), an instantiation of A is matched with the one of B that has a 0 there.  A stream that differs only in the
offsets of kernel-argument loads and the kernel-argument size (the argument struct grew: what lies behind it moved) is reported as such.
Other kernels are labelled by their demangled names (c++filt) and matched by name, or through RENAMED below.
profiles/ball_joints_codegen.txt, profiles/reset_noise_codegen.txt and profiles/rowpass_split_codegen.txt are its output."""
import re
import subprocess
import sys

SOURCE = sys.argv[3] if len(sys.argv) > 3 else "k_physics"
KERNELS = sys.argv[4] if len(sys.argv) > 4 else "env_kernel"
# kernels of tree A that tree B has under another name: the gather-only launch used to be the <ROLLOUT, PRE> instantiations of fused_mlp_kernel
RENAMED = {"_ZN4mppo16fused_mlp_kernelILb0ELb1ELi1ELb1ELb1ELi1EEEvNS_9FusedArgsE": "_ZN4mppo18gather_rows_kernelILb0EEEvNS_9FusedArgsE",
           "_ZN4mppo16fused_mlp_kernelILb1ELb1ELi1ELb1ELb1ELi1EEEvNS_9FusedArgsE": "_ZN4mppo18gather_rows_kernelILb1EEEvNS_9FusedArgsE"}


def funcs(path):
    out, cur, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_ZN4mppo\d+(?:" + KERNELS + r")I\S+):\s", line)
        if m:
            cur, body = m.group(1), []
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                out[cur], cur = body, None
                continue
            t = line.split(";")[0].rstrip()
            if not t.strip():
                continue
            t = re.sub(r"\.LBB\d+_", ".LBB_", t)
            t = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", t)
            t = re.sub(r"_ZN4mppo\S+", "SYM", t)
            body.append(t)
    return out


def remarks(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: (.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].strip()
            out[cur] = {}
        elif cur and ":" in t:
            k, v = t.split(":", 1)
            out[cur][k.strip()] = v.strip()
    return out


def dims(name):
    m = re.search(r"StaticModelI((?:Li\d+E)+)EELi(\d)E", name)
    if not m:
        return None
    return tuple(int(x) for x in re.findall(r"Li(\d+)E", m.group(1))), int(m.group(2))


def label(name):
    d = dims(name)
    if d:
        return f"StaticModel{d[0]} mode {d[1]}"
    m = re.search(r"(Runtime\w*Model)ELi(\d)E", name)
    return f"{m.group(1)} mode {m.group(2)}" if m else demangled(name)


def demangled(name):
    try:
        return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().replace("void mppo::", "").replace("(mppo::FusedArgs)", "") or name
    except FileNotFoundError:
        return name


def verdict(a, b):
    if a == b:
        return "IDENTICAL", True
    if len(a) == len(b):
        bad = [(x, y) for x, y in zip(a, b) if x != y]
        arg = lambda t: re.sub(r"0x[0-9a-f]+\s*$", "OFF", t) if re.match(r"\s*s_load_dword", t) else re.sub(r"\d+\s*$", "N", t) if ".amdhsa_kernarg_size" in t else t
        if all(arg(x) == arg(y) for x, y in bad):
            return f"IDENTICAL but for {len(bad)} kernel-argument offsets / the kernel-argument size", True
        return f"DIFFER in {len(bad)} lines", False
    return "DIFFER", False


old, new = funcs(f"{sys.argv[1]}/{SOURCE}.s"), funcs(f"{sys.argv[2]}/{SOURCE}.s")
ro, rn = remarks(sys.argv[1] + "/remarks.txt"), remarks(sys.argv[2] + "/remarks.txt")
keys = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]", "VGPRs Spill", "SGPRs Spill")
short = lambda r: " ".join(f"{k.split(' [')[0].replace(' ', '')}={r.get(k, '?')}" for k in keys)
newby = {dims(n): n for n in new if dims(n)}
env = KERNELS == "env_kernel"
flags = "-ffp-contract=off" if env else "-ffp-contract=fast"
print(f"# {KERNELS.replace('|', ', ')} instantiations of {SOURCE}.hip, parent commit against this tree: hipcc --offload-arch=gfx950 -O3 -std=c++17 {flags}")
print("# --cuda-device-only -S -Rpass-analysis=kernel-resource-usage; instruction streams compared line by line after dropping comments and")
print("# renumbering local labels.")
MODES = ("reset", "step", "probe", "pushed step", "pushed probe", "split step")  # env_kernel's KMODE
same = {m: [0, 0] for m in range(len(MODES))}
matched = set()
for n in sorted(old, key=label):
    d = dims(n)
    nn = n if n in new else RENAMED.get(n) if RENAMED.get(n) in new else None
    if nn is None and d is not None and len(d[0]) == 16:  # (tree B's names carry the number of ball joints)
        nn = newby.get((d[0][:15] + (0,) + d[0][15:], d[1]))
    if nn is None:
        print(label(n), "MISSING in the new tree")
        continue
    matched.add(nn)
    what, eq = verdict(old[n], new[nn])
    mode = int(label(n)[-1]) if env else 0
    same[mode][0] += eq
    same[mode][1] += 1
    print(f"{label(n)}{'' if nn == n else ' -> ' + label(nn)}\n   parent: {len(old[n])} instructions/directives  {short(ro.get(n, {}))}\n   new   : {len(new[nn])} instructions/directives  {short(rn.get(nn, {}))}\n"
          f"   instruction streams {what}")
for n in sorted(set(new) - matched, key=label):
    print(f"{label(n)} (new)\n   new   : {len(new[n])} instructions/directives  {short(rn.get(n, {}))}")
if env:
    for mode, (s, t) in same.items():
        if t:
            print(f"# mode {mode} ({MODES[mode]}): {s} of {t} instantiations identical to the parent's (kernel-argument offsets aside)")
    print("# scratch bytes per lane, every env_kernel of the new tree:", sorted({rn[n].get("ScratchSize [bytes/lane]") for n in rn if "env_kernel" in n}))
else:
    print(f"# {same[0][0]} of {same[0][1]} instantiations identical to the parent's (kernel-argument offsets aside)")
