"""Spill traffic inside the STEP LOOP of every fan-kernel instance, two builds side by side: instructions, v_readlane /
v_writelane (SGPR spill reloads / stores) and scratch accesses, from hipcc's -save-temps assembly.  scripts/kernel_resources.py
gives the whole kernel's totals; this says whether a change cost the loop anything.
The loop is taken from the CONTROL-FLOW GRAPH, not from the layout: the blocks that are reached from the stage block (the block
with the attempt's table reads) AND reach it, in both cases without passing the service gate (the block with the s_bcnt1 of the
parked-lane count).  Blocks laid out of line -- in front of the loop header or far behind the gate -- count like inline ones.
usage: python scripts/step_loop_spills.py <dir-with-.s of the parent> <dir-with-.s of the new build> [--where]
(--where: for every instance, the blocks of each build's loop that hold v_readlane / v_writelane / scratch accesses)"""
import collections, re, sys
NAME = "/pgr_hip-hip-amdgcn-amd-amdhsa-gfx950.s"
READS = ("ds_read_b128", "global_load_dwordx4")


def blocks_of(body):
    """[(label, [instructions])] and the successor sets (branch targets + fall-through)"""
    blocks, cur = [], ["entry", []]
    blocks.append(cur)
    for l in body:
        t = l.strip()
        if not t or t.startswith((";", "//")):
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            cur = [m.group(1), []]
            blocks.append(cur)
            continue
        if t.startswith(".") or re.match(r"^_Z\S+:", t):
            continue
        cur[1].append(t.split(";")[0].strip())
    idx = {b[0]: i for i, b in enumerate(blocks)}
    succ = []
    for i, (_, ins) in enumerate(blocks):
        out = set()
        for t in ins:
            m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", t)
            if m:
                out.add(idx[m.group(1)])
        last = ins[-1] if ins else ""
        if not last.startswith(("s_branch", "s_endpgm")) and i + 1 < len(blocks):
            out.add(i + 1)
        succ.append(out)
    return blocks, succ


def reach(start, edges, stop):
    seen, todo = {start}, [start]
    while todo:
        for j in edges[todo.pop()]:
            if j not in seen and j not in stop:
                seen.add(j)
                todo.append(j)
    return seen


def scan(path):
    L = open(path + NAME).read().split("\n")
    out = {}
    for a in [i for i, l in enumerate(L) if l.startswith("_Z14pgr_fan_kernelIL") and "; @" in l]:
        m = re.search(r"ILb(\d)ELi(\d)ELi(\d)ELb(\d)ELb(\d)E", L[a])
        body = L[a:a + [i for i, l in enumerate(L[a:]) if l.startswith("\ts_endpgm")][0]]
        blocks, succ = blocks_of(body)
        pred = [set() for _ in blocks]
        for i, s in enumerate(succ):
            for j in s:
                pred[j].add(i)
        nreads = [sum(1 for t in ins if t.startswith(READS)) for _, ins in blocks]
        # the stage block: the FIRST block of the kernel with the most table reads (a replay in the service, where there is one, comes later)
        stage = nreads.index(max(nreads))
        gates = {i for i, (_, ins) in enumerate(blocks) if any(t.startswith("s_bcnt1_i32_b64") for t in ins)}
        loop = reach(stage, succ, gates) & reach(stage, pred, gates)
        c, where = collections.Counter(), {}
        for i in sorted(loop):
            for t in blocks[i][1]:
                op = t.split()[0]
                c[op] += 1
                if op in ("v_readlane_b32", "v_writelane_b32") or "scratch" in op:
                    where.setdefault(blocks[i][0], collections.Counter())[op] += 1
        out[m.groups()] = ((sum(c.values()), c["v_readlane_b32"], c["v_writelane_b32"], sum(v for k, v in c.items() if "scratch" in k)), where)
    return out


P, N = scan(sys.argv[1]), scan(sys.argv[2])
more = 0
print("instance: (instructions, v_readlane, v_writelane, scratch accesses) of the step loop's blocks (control-flow graph), parent -> new")
for k in sorted(P):
    p, n = P[k][0], N[k][0]
    worse = n[1] > p[1] or n[2] > p[2] or n[3] > p[3]
    more += worse
    print("LT %s ZM %s SAVE %s PERSIST %s LOG %s" % k, p, "->", n, "  more spill traffic" if worse else "")
    if "--where" in sys.argv:
        for side, r in (("parent", P[k][1]), ("new", N[k][1])):
            print("      %s:" % side, ", ".join("%s %s" % (b, " ".join("%s x%d" % (o.replace("_b32", ""), v) for o, v in sorted(w.items()))) for b, w in r.items()) or "-")
print(more, "of", len(P), "instances with more spill traffic in the step loop")
