"""Spill traffic inside the STEP LOOP of every fan-kernel instance, two builds side by side: instructions, v_readlane /
v_writelane (SGPR spill reloads / stores) and scratch accesses between the loop header and the service gate (the s_bcnt1 of
the parked-lane count), from hipcc's -save-temps assembly.  scripts/kernel_resources.py gives the whole kernel's totals;
this says whether a change to the service phase cost the loop anything.
usage: python scripts/step_loop_spills.py <dir-with-.s of the parent> <dir-with-.s of the new build>"""
import collections, re, sys
NAME = "/pgr_hip-hip-amdgcn-amd-amdhsa-gfx950.s"


def scan(path):
    L = open(path + NAME).read().split("\n")
    out = {}
    for a in [i for i, l in enumerate(L) if l.startswith("_Z14pgr_fan_kernelIL") and "; @" in l]:
        m = re.search(r"ILb(\d)ELi(\d)ELi(\d)ELb(\d)ELb(\d)E", L[a])
        body = L[a:a + [i for i, l in enumerate(L[a:]) if l.startswith("\ts_endpgm")][0]]
        hs = [i for i, l in enumerate(body) if "Loop Header: Depth=" in l]
        g = [i for i, l in enumerate(body) if "s_bcnt1_i32_b64" in l and i > 1200][0]
        h = max(x for x in hs if x < g - 1000)     # (the latest loop header that has the whole attempt between it and the gate)
        c = collections.Counter(l.split()[0] for l in body[h:g] if l.startswith("\t") and not l.strip().startswith(";"))
        out[m.groups()] = (sum(c.values()), c["v_readlane_b32"], c["v_writelane_b32"], sum(v for k, v in c.items() if "scratch" in k))
    return out


P, N = scan(sys.argv[1]), scan(sys.argv[2])
more = 0
print("instance: (instructions, v_readlane, v_writelane, scratch accesses) from the step loop's header to the service gate, parent -> new")
for k in sorted(P):
    p, n = P[k], N[k]
    worse = n[1] > p[1] or n[2] > p[2] or n[3] > p[3]
    more += worse
    print("LT %s ZM %s SAVE %s PERSIST %s LOG %s" % k, p, "->", n, "  more spill traffic" if worse else "")
print(more, "of", len(P), "instances with more spill traffic in the step loop")
