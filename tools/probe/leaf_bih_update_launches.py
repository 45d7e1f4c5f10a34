"""The launches of the leaf bih updates, for a kernel trace: one triangle bih update and one sphere bih update, each plain and with
glome_scene_nested_updates on (then the refits above), over the tests' fixtures, blocking fp64 host forms.
  rocprofv3 --kernel-trace -d OUT --output-format csv -- python tools/probe/leaf_bih_update_launches.py     (from the repository root)
  python tools/probe/leaf_bih_update_launches.py compare OUT_A OUT_B     the two traces side by side: kernel, grid in lanes, block
(profiles/leaf_bih_refactor_launches.txt: OUT_A from a checkout of the parent commit, OUT_B from the change)."""
import csv
import glob
import re
import sys


def workload():
    sys.path.insert(0, ".")
    sys.path.insert(0, "tests")
    import bihs_refit as BR
    import nested_refit as NR
    import spheres_refit as SR
    from glome_amd import api

    ctx = api.Context(0)
    # plain: the tests' fixtures `mixed` (triangles) and `cluster` (spheres), host forms, fp64
    sd, b, nm, tree = BR.build("mixed", "V0", "tex")
    sc = ctx.commit(b, nm[sd.root])
    assert sc.bih_update(tree, BR.triangles("mixed", "V1")) > 0
    sc.release()
    A = SR.build("cluster", "V0", "tex")
    sc = ctx.commit(A.b, A.root)
    assert sc.sphere_bih_update(A.tree, SR.spheres("cluster", "V1")) > 0
    sc.release()
    # nested: the triangle bih under two trees (test_nested_update_gpu.py), the sphere bih under two trees (test_sphere_bih_update_gpu.py)
    b = api.Builder()
    t = b.bih(b.triangles_bulk(NR.tris9()))
    mid = b.bih([t, b.sphere((2.0, 1.0, -1.0), 0.5), b.sphere((4.0, 2.0, 2.0), 0.4), b.sphere((2.0, 3.0, 3.0), 0.3)])
    top = b.bih([mid, b.sphere((-3.0, 1.0, 0.0), 0.5), b.sphere((0.0, 1.0, -4.0), 0.5), b.sphere((0.0, 5.0, 0.0), 0.5)])
    sc = ctx.commit(b, top)
    sc.nested_updates(True)
    assert sc.bih_update(t, NR.pose_points(NR.tris9().reshape(-1, 3), "grow").reshape(-1, 9)) > 0
    assert sc.refit_above(t) > 0
    sc.release()
    A = SR.build_nested("cluster", "V0", "direct")
    sc = ctx.commit(A.b, A.root)
    sc.nested_updates(True)
    assert sc.sphere_bih_update(A.tree, SR.spheres("cluster", "V1")) > 0
    for tr in sc.bihs_above(A.tree):
        assert sc.bih_refit(tr) > 0
    sc.release()
    ctx.close()
    print("launches done")


def load(d):
    f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    assert len(f) == 1, f
    rows = list(csv.DictReader(open(f[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = []
    for r in rows:
        name = re.sub(r"\(.*$", "", r["Kernel_Name"]).replace("void ", "").replace("glome::", "")
        name = re.sub(r"\.kd$", "", name)
        out.append((name, int(r["Grid_Size_X"]) * int(r.get("Grid_Size_Y", 1) or 1) * int(r.get("Grid_Size_Z", 1) or 1), int(r["Workgroup_Size_X"])))
    return out


def compare(a, b):
    P, C = load(a), load(b)
    upd = ("upd::", "meshupd::", "bihupd::", "sphupd::", "itemupd::")
    print(f"dispatches: A {len(P)}, B {len(C)}")
    diff = 0
    for k in range(max(len(P), len(C))):
        a = P[k] if k < len(P) else ("-", 0, 0)
        b = C[k] if k < len(C) else ("-", 0, 0)
        diff += a != b
        if a[0].startswith(upd) or b[0].startswith(upd) or a != b:
            print(f"{k:4}  {a[0][:60]:<60} {a[1]:>6} {a[2]:>4} | {b[0][:60]:<60} {b[1]:>6} {b[2]:>4}{'   <-- differs' if a != b else ''}")
    print(f"rows that differ: {diff} of {max(len(P), len(C))} (not listed: the commit-time and runtime-internal kernels, equal in name and size row for row)")


if __name__ == "__main__":
    compare(*sys.argv[2:4]) if sys.argv[1:2] == ["compare"] else workload()
