"""Where are a live item's instructions: in the two hand-written walks, or in the compiler's code around them?  A MODEL, not a count: the
events of the wave-wide walks per live item of the S3 frame (tools/probe/bih_cull_study.cpp, its EVENTS line: branch steps, pushes, leaf
visits and pair tests of the primary and of the shadow walk, counted on the CPU per 8 x 8 packet) times the instructions each event
costs, read here from the flagship kernel's listing (tools/kernel_mix.py 1 leaves it in its output directory): the labels of an inlined
walk block (bih_packet_asm.hpp) cut it into the step variants L_st* / L_nf* / L_fo* (before round 11: L_n1*, and L_node for the far
child's fetch), the pair test L_tri .. L_pop and the pop L_pop .. L_empty.  What the counters give for a live item
(tools/probe/item_overhead.py --pmc ... --live N) less the model's walks is what lies outside them.

A branch step is priced by its KIND, each by its own path through the listing (the EVENTS line's near_only / far_only / both / neither:
which children the packet's rays go into):
  near only   L_st up to the far vote, then L_nf
  neither     L_st up to the far vote, the near vote and its branch to the pop (the pop itself is not charged: see below)
  both        the whole of L_st: both votes, the capacity test, the push, the near child's dispatch (before round 11: L_st with its push,
              then L_nf)
  far only    L_st up to the near vote's branch, then L_fo (before round 11: L_st WITH its push, the near vote, L_n1 which takes the push
              back, L_node's wait and fetch and its dispatch)
A dispatch is counted at its longest path (five instructions; four or two are executed for three of the four targets).  An EVENTS line
without the four kinds (older than round 11) is priced as before: one figure per step, the push where both children are entered -- which
charged the parent's far-only steps 15 instructions too few each and put them into "outside the walks".

Pops are charged per push (pops = pushes): every entry pushed is popped once.  The pop that finds the stack empty and ends a walk -- one
per walk that left its root branch -- is charged nowhere, so the model's walks are short by up to one pop (20 instructions) per walk,
about 40 per live item, which the "outside" figure holds instead.

  g++ -O2 -std=c++17 -I glome_amd/csrc -I include tools/probe/bih_cull_study.cpp -o BUILD/bih_cull_study && BUILD/bih_cull_study 224 8 3 | grep EVENTS > BUILD/events.txt
  python tools/kernel_mix.py 1 > /dev/null
  python tools/probe/item_breakdown.py BUILD/events.txt [--listing FILE.s] [--kernel MANGLED] [--counted 4636.2]
(BUILD: any directory outside the tree's tracked files)
"""
import json
import re
import sys

LISTING = "/tmp/kernel_mix/p1/kernel_parts-hip-amdgcn-amd-amdhsa-gfx950.s"  # where tools/kernel_mix.py 1 writes it
KERNEL = "_Z13k_render_flatILb0ELb0ELb0ELi1ELi6ELb1EEvN5glome11DRenderArgsEiPji"  # the flagship instance


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def kernel_lines(path, kernel):
    out, on = [], False
    for line in open(path):
        s = line.strip()
        if s.startswith(kernel + ":"):
            on = True
            continue
        if on:
            if s.startswith("s_endpgm"):
                break
            if s and not s.startswith((";", ".")):
                out.append(s)
    return out


def is_label(s):
    return s.endswith(":")


def main():
    ev = json.loads(open(sys.argv[1]).read().split("EVENTS", 1)[1])
    lines = kernel_lines(arg("--listing", LISTING), arg("--kernel", KERNEL))
    total = sum(1 for s in lines if not is_label(s))
    # the walk blocks: L_fresh_N .. L_end_N
    blocks, cur = {}, None
    inside = 0
    for s in lines:
        m = re.match(r"L_fresh_(\d+):", s)
        if m:
            cur = m.group(1); blocks[cur] = []
        if cur is not None:
            blocks[cur].append(s)
            inside += 0 if is_label(s) else 1
            if s == f"L_end_{cur}:":
                cur = None
    # one block's segments (every block has the same shape; the mean over the blocks is reported)
    cost = {"step": [], "push": [], "near_only": [], "far_only": [], "both": [], "neither": [], "pair": [], "pop": [], "leaf_entry": []}
    for n, b in blocks.items():
        seg, name = {}, None
        for s in b:
            if is_label(s):
                name = s[:-1]; seg[name] = []
            elif name:
                seg[name].append(s)
        st = [k for k in seg if k.startswith("L_st")]
        if not st:
            continue
        for k in st:
            tag = k[len("L_st"):]
            body = seg[k]
            cut = next(i for i, s in enumerate(body) if s.startswith("s_cbranch_vccz L_nf")) + 1  # up to the vote "does any lane enter the far child"
            nf = seg["L_nf" + tag]
            vote = next(i for i, s in enumerate(nf) if s.startswith("s_cbranch_execz")) + 1  # the near vote and its branch
            cost["step"].append(cut + len(nf))
            cost["near_only"].append(cut + len(nf))
            if "L_fo" + tag in seg:  # the far child entered alone is a step of its own
                fo = next(i for i, s in enumerate(body) if s.startswith("s_cbranch_scc0 L_fo")) + 1
                cost["push"].append(len(body) - cut - (len(nf) - vote))  # (what a step that pushes costs beyond a near-only one)
                cost["both"].append(len(body))
                cost["far_only"].append(fo + len(seg["L_fo" + tag]))
                cost["neither"].append(cut + vote)
            else:  # it is pushed and taken back, and its node fetched through L_node
                cost["push"].append(len(body) - cut)
                cost["both"].append(len(body) + len(nf))
                cost["far_only"].append(len(body) + vote + len(seg["L_n1" + tag]) + len(seg[f"L_node_{n}"]) + len(seg[f"L_node2_{n}"]))
                cost["neither"].append(cut + vote + 1)
        cost["pair"].append(len(seg[f"L_tri_{n}"]))
        cost["pop"].append(len(seg[f"L_pop_{n}"]))
        cost["leaf_entry"].append(len(seg[f"L_leaf_{n}"]) + len(seg.get(f"L_zlA_{n}", [])))
    c = {k: sum(v) / len(v) for k, v in cost.items()}
    rows, walks = [], 0.0
    for w in ("primary", "shadow"):
        e = ev[w]
        if "far_only" in e:
            parts = {k.replace("_", " ") + " steps": e[k] * c[k] for k in ("near_only", "far_only", "both", "neither")}
        else:
            parts = {"branch steps": e["branch_steps"] * c["step"], "pushes": e["pushes"] * c["push"]}
        parts.update({"pops": e["pushes"] * c["pop"], "pair tests": e["pair_tests"] * c["pair"], "leaf entries": e["leaf_visits"] * c["leaf_entry"]})
        rows.append((w, e, parts))
        walks += sum(parts.values())
    print(f"listing: {total} instructions, {inside} inside the {len(blocks)} walk blocks, {total - inside} outside")
    print("per event (listing): " + ", ".join(f"{k} {v:.1f}" for k, v in c.items()))
    print(f"events per live item ({ev['live_items']} live of {ev['items_sampled']} sampled items):")
    for w, e, parts in rows:
        kinds = "  (near only {near_only:.1f}, far only {far_only:.1f}, both {both:.1f}, neither {neither:.1f})".format(**e) if "far_only" in e else ""
        print(f"  {w:8s} walks {e['walks']:.2f}  steps {e['branch_steps']:.1f}{kinds}  pushes = pops {e['pushes']:.1f}  leaf visits {e['leaf_visits']:.1f}  pair tests {e['pair_tests']:.1f}")
        print("           instructions: " + ", ".join(f"{k} {v:.0f}" for k, v in parts.items()) + f"  = {sum(parts.values()):.0f}")
    print(f"in the walks (model): {walks:.0f} per live item")
    if "--counted" in sys.argv:
        counted = float(arg("--counted", "0"))
        print(f"counted: {counted:.1f} per live item -> outside the walks: {counted - walks:.0f} ({100 * (counted - walks) / counted:.0f} %)")


if __name__ == "__main__":
    main()
