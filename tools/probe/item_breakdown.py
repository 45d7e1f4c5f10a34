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
A dispatch -- the branch on a reference's two low bits that ends every step and every pop -- is priced by WHERE IT GOES when the study's
TRANS line is given (--trans FILE: per site -- after an X / Y / Z step, after a pop, at the root -- how many dispatches go to an X, Y, Z
branch and to a leaf, per live item): the instructions executed on that path through the site's own form (DISPATCH_PATHS below, read off
bih_packet_asm.hpp: since round 12 every site has its own test order; before, one form served all), and the step kinds and the pop are
priced WITHOUT their dispatch.  Without --trans a dispatch is counted at its full length inside the step, as until round 11.  An EVENTS line
without the four kinds (older than round 11) is priced as before: one figure per step, the push where both children are entered -- which
charged the parent's far-only steps 15 instructions too few each and put them into "outside the walks".

A pair test is priced by its PATH when the study's PAIRS line is given (--pairs FILE: per walk the pair tests, those where some entering
ray has b1 in [0, 1] for A or B, the triangles tested and those some ray hits): since round 13 a test no ray can pass leaves after b1
(L_tri up to the vote's branch, then L_out: 2 instructions when the pair was the leaf's last -- leaf visits / pair tests of them --, else 4),
the others run through (L_tri, L_noA, L_noB), and the closest-hit walk's update (3 vector instructions) is charged per triangle HIT.  The primary
walk is priced from the closest-hit blocks (those with an s_cbranch_execz over the update), the shadow walk from the any-hit blocks; a
listing without L_out (the parent's) is priced whole for every test.  The line "pair tests by kind" splits the sum into vector instructions
and the rest: the fall of the first is what SQ_INSTS_VALU should show.

Pops are charged per push (pops = pushes): every entry pushed is popped once.  The pop that finds the stack empty and ends a walk -- one
per walk that left its root branch -- is charged nowhere, so the model's walks are short by up to one pop (20 instructions) per walk,
about 40 per live item, which the "outside" figure holds instead.

  g++ -O2 -std=c++17 -I glome_amd/csrc -I include tools/probe/bih_cull_study.cpp -o BUILD/bih_cull_study && BUILD/bih_cull_study 224 8 3 | grep EVENTS > BUILD/events.txt
  python tools/kernel_mix.py 1 > /dev/null
  python tools/probe/item_breakdown.py BUILD/events.txt [--trans BUILD/trans.txt] [--pairs BUILD/pairs.txt] [--listing FILE.s] [--kernel MANGLED] [--counted 4636.2]
(BUILD: any directory outside the tree's tracked files)
"""
import json
import re
import sys

LISTING = "/tmp/kernel_mix/p1/kernel_parts-hip-amdgcn-amd-amdhsa-gfx950.s"  # where tools/kernel_mix.py 1 writes it
KERNEL = "_Z13k_render_flatILb0ELb0ELb0ELi1ELi6ELb1EEvN5glome11DRenderArgsEiPji"  # the flagship instance


# instructions executed by a dispatch, by site and target (x, y, z, leaf), and the site's length in the listing.  "r12": the per-site forms
# (a block that has the label L_xyA); "r11": the one form of rounds 2 to 11 (bit 1, then bit 0; s_branch to X and to Z).
DISPATCH_PATHS = {"r12": {"after_x": (5, 4, 4, 4), "after_y": (2, 7, 4, 6), "after_z": (2, 4, 7, 6), "after_pop": (4, 4, 4, 5), "at_root": (4, 4, 4, 4)},
                  "r11": {k: (5, 4, 5, 4) for k in ("after_x", "after_y", "after_z", "after_pop")}}
DISPATCH_PATHS["r11"]["at_root"] = (4, 4, 5, 4)  # (the root's form fell through into the X step)
DISPATCH_LEN = {"r12": {"X": 5, "Y": 7, "Z": 7, "pop": 5}, "r11": {"X": 5, "Y": 5, "Z": 5, "pop": 5}}


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
    ev = json.loads(open(sys.argv[1]).read().split("EVENTS", 1)[1].splitlines()[0])
    pairs = json.loads(open(arg("--pairs", "")).read().split("PAIRS", 1)[1].splitlines()[0]) if "--pairs" in sys.argv else None
    pair_paths = {1: [], 2: []}  # per mode: (early, full without updates, update) as (all, vector) instruction counts per block
    trans = json.loads(open(arg("--trans", "")).read().split("TRANS", 1)[1].splitlines()[0]) if "--trans" in sys.argv else None
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
        form = "r12" if f"L_xyA_{n}" in seg else "r11"
        for k in st:
            tag = k[len("L_st"):]
            body = seg[k]
            if trans:  # the three dispatches of a step (both, near only, far only) leave: they are priced by where they go
                cutd = DISPATCH_LEN[form][tag[1]]
                seg["L_nf" + tag] = seg["L_nf" + tag][:-cutd]; seg["L_fo" + tag] = seg["L_fo" + tag][:-cutd]; body = body[:-cutd]
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
        tri = seg[f"L_tri_{n}"]
        nv = lambda ls: sum(1 for x in ls if x.startswith("v_"))
        if f"L_out_{n}" in seg:  # round 13: the test in two parts
            full = tri + seg[f"L_noA_{n}"] + seg[f"L_noB_{n}"]
            mode = 1 if any(x.startswith("s_cbranch_execz L_noA") for x in tri) else 2
            vote = next(i for i, x in enumerate(tri) if x.startswith("s_cbranch_scc0 L_out")) + 1
            upd = [x for x in full if x.startswith(("v_mov_b32", "v_add_u32"))] if mode == 1 else []
            pair_paths[mode].append(((vote, nv(tri[:vote])), (len(full) - len(upd), nv(full) - len(upd)), (len(upd) / 2.0, len(upd) / 2.0)))
            cost["pair"].append(len(full))
        else:
            mode = 1 if sum(1 for x in tri if x.startswith("v_mov_b32")) >= 4 else 2
            pair_paths[mode].append(((0, 0), (len(tri), nv(tri)), (0, 0)))
            cost["pair"].append(len(tri))
        cost["pop"].append(len(seg[f"L_pop_{n}"]) - (DISPATCH_LEN[form]["pop"] if trans else 0))
        cost["leaf_entry"].append(len(seg[f"L_leaf_{n}"]) + (0 if trans else len(seg.get(f"L_zlA_{n}", []))))
    c = {k: sum(v) / len(v) for k, v in cost.items()}
    rows, walks, pair_kinds, valu_pairs = [], 0.0, [], [0.0, 0.0]
    for w in ("primary", "shadow"):
        e = ev[w]
        if "far_only" in e:
            parts = {k.replace("_", " ") + " steps": e[k] * c[k] for k in ("near_only", "far_only", "both", "neither")}
        else:
            parts = {"branch steps": e["branch_steps"] * c["step"], "pushes": e["pushes"] * c["push"]}
        parts.update({"pops": e["pushes"] * c["pop"], "pair tests": e["pair_tests"] * c["pair"], "leaf entries": e["leaf_visits"] * c["leaf_entry"]})
        if pairs:
            pw, mode = pairs[w], 1 if w == "primary" else 2
            pp = [[sum(b[i][j] for b in pair_paths[mode]) / len(pair_paths[mode]) for j in (0, 1)] for i in (0, 1, 2)]
            if pp[0][0]:
                last = min(1.0, e["leaf_visits"] / e["pair_tests"])
                n_early, n_full = pw["pair_tests"] - pw["some_ray_b1"], pw["some_ray_b1"]
                tot = [n_early * pp[0][j] + n_full * pp[1][j] + pw["triangles_hit"] * pp[2][j] for j in (0, 1)]
                tot[0] += n_early * (2 * last + 4 * (1 - last))
            else:
                n_early, n_full = 0.0, pw["pair_tests"]
                tot = [n_full * pp[1][j] for j in (0, 1)]
            parts["pair tests"] = tot[0]
            pair_kinds.append(f"  {w:8s} pair tests by path: {n_early:.2f} leave after b1 at {pp[0][0]:.0f} ({pp[0][1]:.0f} vector) + L_out, {n_full:.2f} run through at {pp[1][0]:.0f} ({pp[1][1]:.0f} vector)"
                              f" + {pp[2][0]:.0f} per triangle hit ({pw['triangles_hit']:.2f} of {pw['triangles']:.2f})  -> pair tests by kind: vector {tot[1]:.1f}, the rest {tot[0] - tot[1]:.1f}")
            valu_pairs[0] += tot[1]; valu_pairs[1] += tot[0] - tot[1]
        if trans:
            parts["dispatches"] = sum(n_ * p_ for site, paths in DISPATCH_PATHS[form].items() for n_, p_ in zip(trans[w][site], paths))
        rows.append((w, e, parts))
        walks += sum(parts.values())
    print(f"listing: {total} instructions, {inside} inside the {len(blocks)} walk blocks, {total - inside} outside")
    print("per event (listing): " + ", ".join(f"{k} {v:.1f}" for k, v in c.items()))
    print(f"events per live item ({ev['live_items']} live of {ev['items_sampled']} sampled items):")
    for w, e, parts in rows:
        kinds = "  (near only {near_only:.1f}, far only {far_only:.1f}, both {both:.1f}, neither {neither:.1f})".format(**e) if "far_only" in e else ""
        print(f"  {w:8s} walks {e['walks']:.2f}  steps {e['branch_steps']:.1f}{kinds}  pushes = pops {e['pushes']:.1f}  leaf visits {e['leaf_visits']:.1f}  pair tests {e['pair_tests']:.1f}")
        print("           instructions: " + ", ".join(f"{k} {v:.0f}" for k, v in parts.items()) + f"  = {sum(parts.values()):.0f}")
    if trans:
        for site, paths in DISPATCH_PATHS[form].items():
            counts = [trans["primary"][site][t] + trans["shadow"][site][t] for t in range(4)]
            print(f"  dispatches {site:9s} -> x {counts[0]:.2f} y {counts[1]:.2f} z {counts[2]:.2f} leaf {counts[3]:.2f}  at {paths}: {sum(a * b for a, b in zip(counts, paths)):.1f}")
    for line in pair_kinds:
        print(line)
    if pair_kinds:
        print(f"pair tests of both walks (model): vector {valu_pairs[0]:.1f}, the rest {valu_pairs[1]:.1f} per live item")
    print(f"in the walks (model): {walks:.0f} per live item")
    if "--counted" in sys.argv:
        counted = float(arg("--counted", "0"))
        print(f"counted: {counted:.1f} per live item -> outside the walks: {counted - walks:.0f} ({100 * (counted - walks) / counted:.0f} %)")


if __name__ == "__main__":
    main()
