"""The generic tier's frame-memory estimate against the words the interpreter writes, per frame kind and bottom (no GPU: the host build of the
device headers, tests/hostsim; the scenes of tests/frame_towers.py).   usage: python tools/probe/frame_words.py > profiles/frame_words.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import frame_towers as FT  # noqa: E402

K = FT.K
DOWN = (np.array([[FT.BOTTOM_XY[0], FT.BOTTOM_XY[1], FT.Z_START]], np.float32), FT.tilted()[None], 64.0)


def per_level(kind, bot, route):
    e, w = [], []
    for n in (3, 4):
        hs = FT.commit_host(FT.tower(kind, bot, n).sd)[0]
        if kind in FT.WARP_KINDS:  # (the tower is reached from the shader alone: the trace route, whichever column)
            w.append(int(hs.frame_probe("trace", DOWN[0], DOWN[1], 1e6, lights=FT.LIGHTS, maxdepth=2)["words"][0]))
        else:
            w.append(int(hs.frame_probe(route, *DOWN)["words"][0]))
        e.append(hs.vm_words()[0])
    return e[1] - e[0], w[1] - w[0]


print("Frame words per ray of the generic tier: the commit-time estimate (flatten.hpp vm_words_of) against the words the interpreter writes")
print("(rt_generic.hpp, host build; tests/test_frame_words_host.py holds every figure).  kVmWords = %d; written words are a lower bound of the" % K["kVmWords"])
print("stack height (a frame reserves words it may never write); per level = from L to L + 1 levels of the kind, under one ray down the tower.")
print("constants: " + ", ".join("%s %d" % kv for kv in K.items()))
print()
print("%-11s %-10s | %9s %9s %6s | %9s %9s %6s | %-14s %5s %7s" % ("kind", "bottom", "est/level", "written", "slack", "est/level", "written", "slack", "brim (k, x, ib)", "est", "left"))
print("%-11s %-10s | %28s | %28s |" % ("", "", "rayint route", "shadow route"))
for kind, bot in FT.BRIMS:
    if bot in FT.FAMILIES: continue
    er, wr = per_level(kind, bot, "rayint")
    es, ws = per_level(kind, bot, "shadow")
    b = FT.brim(kind, bot)
    est = FT.estimate(FT.tower(kind, bot, *b).sd)
    print("%-11s %-10s | %9d %9d %6d | %9d %9d %6d | %-14s %5d %7d" % (kind, bot, er, wr, er - wr, es, ws, es - ws, "%d, %d, %d" % b, est, K["kVmWords"] - est))
print()
print("warp_frame / warp_scene: a group [transform] tower that is the frame / the scene of a Warp material on a disc; both columns are the trace route at")
print("maxdepth 2 (rayint and shadow of the root never reach the tower), the estimate is the Warp roots' (flatten.hpp bind_warps), carried by FlatScene::vm_words.")
print("brim (k, x, ib): k levels of the kind, then x levels of group [transform] and ib bare innerbound levels as filler; one innerbound more is refused.")
print()
print("The advance families under group [transform] levels (estimate and written words at 0 levels; the brim under xform levels):")
print("%-11s %5s %9s | %-44s | %-14s %5s | %s" % ("family", "est", "allowance", "steps of a ray: words written", "brim (k, x, ib)", "est", "first flagged at the brim"))
for bot in FT.FAMILIES:
    tw, hs, est, o, d, tm, cnt = FT.family(bot, 0)
    p = hs.frame_probe("rayint", o, d, tm)
    order = np.argsort(cnt, kind="stable")
    c, w = cnt[order], p["words"][order]
    a = FT.ALLOWANCE[bot]
    pick = sorted(set([int(c.min()), a, int(c.max())]))
    steps = ", ".join("%d: %d" % (k, int(w[c == k][0])) for k in pick if (c == k).any())
    b = FT.brim("xform", bot)
    twb = FT.tower("xform", bot, *b)
    hb = FT.commit_host(twb.sd)[0]
    ob, db, tmb, cb = FT.FAMILY_RAYS[bot](twb.shift)
    pb = hb.frame_probe("rayint", ob, db, tmb)
    first = "%d steps" % int(cb[pb["flag"]].min()) if pb["flag"].any() else "none (the unused frames of the allowance hold every ray)"
    print("%-11s %5d %9d | %-44s | %-14s %5d | %s" % (bot, est, a, steps, "%d, %d, %d" % b, hb.vm_words()[0], first))
print()
print("steps: advances of the Difference (carve, carve_mesh: 1 word each), advances of the Intersection (chain, chain2: kVmIsectWords each), children the ray")
print("leaves with no advance (chain_in: kVmIsectWords each, counted at commit).  No ray wrote past the frame memory (64 canary words, two sentinels).")
