"""Where are a live item's instructions: in the two hand-written walks, or in the compiler's code around them?  A MODEL, not a count: the
events of the wave-wide walks per live item of the S3 frame (tools/probe/bih_cull_study.cpp, its EVENTS line: branch steps, pushes, leaf
visits and pair tests of the primary and of the shadow walk, counted on the CPU per 8 x 8 packet) times the instructions each event
costs, read here from the flagship kernel's listing (tools/kernel_mix.py 1 leaves it in its output directory): the labels of an inlined
walk block (bih_packet_asm.hpp) cut it into the step variants L_st* / L_nf* / L_n1*, the pair test L_tri .. L_pop and the pop
L_pop .. L_empty.  What the counters give for a live item (tools/probe/item_overhead.py --pmc ... --live N) less the model's walks is
what lies outside them.

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
    cost = {"step": [], "push": [], "pair": [], "pop": [], "leaf_entry": []}
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
            cost["step"].append(cut + len(seg["L_nf" + tag]))
            cost["push"].append(len(body) - cut)
        cost["pair"].append(len(seg[f"L_tri_{n}"]))
        cost["pop"].append(len(seg[f"L_pop_{n}"]))
        cost["leaf_entry"].append(len(seg[f"L_leaf_{n}"]) + len(seg.get(f"L_zlA_{n}", [])))
    c = {k: sum(v) / len(v) for k, v in cost.items()}
    rows, walks = [], 0.0
    for w in ("primary", "shadow"):
        e = ev[w]
        parts = {"branch steps": e["branch_steps"] * c["step"], "pushes": e["pushes"] * c["push"], "pops": e["pushes"] * c["pop"],
                 "pair tests": e["pair_tests"] * c["pair"], "leaf entries": e["leaf_visits"] * c["leaf_entry"]}
        rows.append((w, e, parts))
        walks += sum(parts.values())
    print(f"listing: {total} instructions, {inside} inside the {len(blocks)} walk blocks, {total - inside} outside")
    print("per event (listing): " + ", ".join(f"{k} {v:.1f}" for k, v in c.items()))
    print(f"events per live item ({ev['live_items']} live of {ev['items_sampled']} sampled items):")
    for w, e, parts in rows:
        print(f"  {w:8s} walks {e['walks']:.2f}  steps {e['branch_steps']:.1f}  pushes = pops {e['pushes']:.1f}  leaf visits {e['leaf_visits']:.1f}  pair tests {e['pair_tests']:.1f}")
        print("           instructions: " + ", ".join(f"{k} {v:.0f}" for k, v in parts.items()) + f"  = {sum(parts.values()):.0f}")
    print(f"in the walks (model): {walks:.0f} per live item")
    if "--counted" in sys.argv:
        counted = float(arg("--counted", "0"))
        print(f"counted: {counted:.1f} per live item -> outside the walks: {counted - walks:.0f} ({100 * (counted - walks) / counted:.0f} %)")


if __name__ == "__main__":
    main()
