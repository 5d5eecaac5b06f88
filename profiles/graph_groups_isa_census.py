#!/usr/bin/env python3
"""profiles/graph_groups_isa_census.py BEFORE.s BEFORE.remarks AFTER.s AFTER.remarks > profiles/graph_groups_isa_census.txt

Registers, scratch, LDS and occupancy of every kernel of csrc/expann_graph.hip before (the parent commit) and after
the row groups, and whether each existing kernel kept its instruction stream.  The inputs come from
  hipcc -O3 --offload-arch=gfx950 -std=c++17 -I include -I include/expann --offload-device-only -S \\
        -Rpass-analysis=kernel-resource-usage expann_amd/csrc/expann_graph.hip -o X.s > X.remarks 2>&1
'isa' compares the instruction lines of the two -S outputs (comments and directives dropped, block labels
renumbered).  The walk's template flag became an int: <.., false, ..> is now <.., 0, ..>, <.., true, ..> is <.., 1, ..>;
the names are matched through that."""
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: [instruction lines]} of the .amdhsa_kernel functions of a -S output"""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        t = line.split(";")[0].rstrip()
        if t.strip() == "s_endpgm":
            out[name] = body + ["s_endpgm"]
            name = None
        elif t.startswith("\t") and not t.strip().startswith("."):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(t.split())))
        elif re.match(r"^\.LBB\d+_\d+:", t):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def resources(path):
    out = {}
    for b in re.split(r"remark: Function Name: ", open(path).read())[1:]:
        g = lambda k: int(re.search(k + r": (\d+)", b).group(1))
        out[b.split()[0]] = (g("TotalSGPRs"), g(r"\bVGPRs"), g("AGPRs"), g(r"ScratchSize \[bytes/lane\]"),
                             g(r"LDS Size \[bytes/block\]"), g(r"Occupancy \[waves/SIMD\]"))
    return out


def old_to_new(name):
    return re.sub(r"(graph_search_kernelILi\d+ELi\dELi\dE)Lb([01])E", r"\1Li\2E", name)


def demangle(names):
    txt = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout
    short = [re.sub(r"^void expann::|\(.*$", "", x) for x in txt.splitlines()]
    return dict(zip(names, short))


def main(before_s, before_r, after_s, after_r):
    kb, ka = kernels(before_s), kernels(after_s)
    rb, ra = resources(before_r), resources(after_r)
    rb = {old_to_new(k): v for k, v in rb.items()}
    kb = {old_to_new(k): v for k, v in kb.items()}
    existing = [k for k in rb if k in ra]
    new = [k for k in ra if k not in rb]
    gone = [k for k in rb if k not in ra]
    same = [k for k in existing if kb.get(k) == ka.get(k)]
    changed = [k for k in existing if k not in same]
    res_changed = [k for k in existing if rb[k] != ra[k]]
    dm = demangle(list(ra) + gone)
    print(__doc__.split("\n\n")[1].replace("\n", "\n"))
    print()
    print(f"kernels before: {len(rb)}   after: {len(ra)}   new: {len(new)}   gone: {len(gone)}")
    print(f"existing kernels, instruction stream unchanged: {len(same)}   changed: {len(changed)}")
    print(f"existing kernels whose registers / scratch / LDS / occupancy changed: {len(res_changed)}")
    print(f"kernels with scratch, before: {sum(1 for v in rb.values() if v[3])}   after: {sum(1 for v in ra.values() if v[3])}")
    hdr = f"{'kernel':72s} {'sgpr':>5s} {'vgpr':>5s} {'agpr':>5s} {'scr':>4s} {'lds':>7s} {'occ':>4s}  isa"
    print("\n-- existing kernels whose instruction stream or resources changed (before -> after) --")
    print(hdr)
    for k in existing:
        if k in changed or k in res_changed:
            print(f"{dm[k]:72s} " + " ".join(f"{a}->{b}" if a != b else str(a) for a, b in zip(rb[k], ra[k])) +
                  f"  {'same' if k in same else f'{len(kb[k])} -> {len(ka[k])} instruction lines'}")
    print("\n-- existing kernels, unchanged --")
    print(hdr)
    for k in existing:
        if k in same and k not in res_changed:
            print(f"{dm[k]:72s} {ra[k][0]:5d} {ra[k][1]:5d} {ra[k][2]:5d} {ra[k][3]:4d} {ra[k][4]:7d} {ra[k][5]:4d}  same")
    print("\n-- new kernels --")
    print(hdr)
    for k in new:
        print(f"{dm[k]:72s} {ra[k][0]:5d} {ra[k][1]:5d} {ra[k][2]:5d} {ra[k][3]:4d} {ra[k][4]:7d} {ra[k][5]:4d}  new")


if __name__ == "__main__":
    main(*sys.argv[1:5])
