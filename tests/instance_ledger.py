"""The ledger of kernel instances: one table, LAUNCHES, with at least one launch for every separately compiled render, sampler and
trace kernel -- the 17 k_render_flat, 9 k_ss_frame_flat and 16 k_trace_batch_flat instances glome_amd/csrc/instances.hpp lists and
the six kernels of the generic tier (render, sampler and trace, each lean and counting).

A plain module: no GPU, no fixtures.  tests/test_instance_ledger.py (no GPU) asserts that every row gets the instance it names and
that the rows name every instance the rules can choose; tests/test_instance_parity.py (GPU) launches every row and compares it
with the oracle.  Both are parametrized from this table and take their cases from nowhere else.

Instance names are the strings test_kernel_choice.instance_name and test_trace_choice.instance_name print:
    k_render_flat<FAITHFUL,COUNT,FULL,CLS,LB,TWO_ROWS>    k_ss_frame_flat<FULL,CLS,LB,TWO_ROWS,FAITHFUL>
    k_trace_batch_flat<FAITHFUL,COUNT,FULL,CLS,LB>        k_*_generic<lean> / <counting>"""
from collections import namedtuple

import zoo
from glome_amd import scenes

RENDER, SAMPLER, TRACE = "render", "sampler", "trace"
# the frame of a row by its kind: a render row's frame, a sampler row's frame, and the frame whose primary rays a trace row traces
FRAME = {RENDER: (320, 180), SAMPLER: (195, 130), TRACE: (192, 108)}

# gpu=False: the row is checked by the CPU test only (its launch is too large for a test of seconds)
Row = namedtuple("Row", "id make kind maxdepth faithful count_work width height instance gpu")

SCENES = {
    "S1": lambda: scenes.s1(nlights=2), "S3small": lambda: scenes.s3(24), "S3mesh_small": lambda: scenes.s3(24, as_mesh=True), "S4": scenes.s4,
    "S5": scenes.CONFIGS["S5"]["make"],
    "flat_mixed": zoo.flat_mixed, "quadrics": zoo.quadrics, "materials": zoo.materials, "textures": zoo.textures, "nested": zoo.nested,
    "mirror_tri": zoo.mirror_tri, "mirror_mesh": zoo.mirror_mesh, "every_class": zoo.every_class,
}
NEW_SCENES = ("mirror_tri", "mirror_mesh", "every_class")  # made for this table (tests/zoo.py): the CPU test checks that they are worth a launch


def _row(kind, scene, maxdepth, instance, faithful=0, count_work=0, gpu=True):
    rid = "%s-%s-d%d%s%s" % (kind, scene, maxdepth, "-faithful" if faithful else "", "-count" if count_work else "")
    return Row(rid, SCENES[scene], kind, maxdepth, faithful, count_work, FRAME[kind][0], FRAME[kind][1], instance, gpu)


def scene_name(row):
    return next(k for k, v in SCENES.items() if v is row.make)


LAUNCHES = [
    # ---------------------------------------------------------------- k_render_flat: production, lean
    _row(RENDER, "mirror_tri", 1, "k_render_flat<false,false,false,TRI,1,false>"),
    _row(RENDER, "S1", 1, "k_render_flat<false,false,false,SPHERE|PRIMS,1,false>"),
    _row(RENDER, "S3mesh_small", 1, "k_render_flat<false,false,false,MESH,1,false>"),
    _row(RENDER, "flat_mixed", 1, "k_render_flat<false,false,false,ALL,1,false>"),
    _row(RENDER, "S3small", 1, "k_render_flat<false,false,false,TRI,6,true>"),
    _row(RENDER, "S3small", 3, "k_render_flat<false,false,false,TRI,6,true>"),
    # ---------------------------------------------------------------- production, full
    _row(RENDER, "mirror_tri", 3, "k_render_flat<false,false,true,TRI,1,false>"),
    _row(RENDER, "S1", 3, "k_render_flat<false,false,true,SPHERE|PRIMS,1,false>"),
    _row(RENDER, "mirror_mesh", 3, "k_render_flat<false,false,true,MESH,1,false>"),
    _row(RENDER, "flat_mixed", 3, "k_render_flat<false,false,true,ALL,1,false>"),
    _row(RENDER, "materials", 1, "k_render_flat<false,false,true,ALL,1,false>"),  # (Blend / AdditiveLayers: full at any depth; Refract, but no ray beyond the primary one)
    # ---------------------------------------------------------------- the CSG class
    _row(RENDER, "every_class", 1, "k_render_flat<false,false,false,EVERY,2,false>"),
    _row(RENDER, "every_class", 3, "k_render_flat<false,false,true,EVERY,2,false>"),
    _row(RENDER, "S4", 1, "k_render_flat<false,false,false,CSG|PRIMS,2,false>"),
    _row(RENDER, "S4", 3, "k_render_flat<false,false,true,CSG|PRIMS,2,false>"),
    _row(RENDER, "quadrics", 3, "k_render_flat<false,false,true,CSG|PRIMS,2,false>"),  # (cylinders and cones: Instances of the canonical quadrics)
    _row(RENDER, "textures", 3, "k_render_flat<false,false,true,CSG|PRIMS,2,false>"),  # (Blend weights from solid textures)
    # ---------------------------------------------------------------- faithful / counting
    _row(RENDER, "S1", 3, "k_render_flat<true,true,true,EVERY,1,false>", faithful=1),
    _row(RENDER, "materials", 3, "k_render_flat<true,true,true,EVERY,1,false>"),  # (a Refract material traced deeper than the primary ray)
    _row(RENDER, "S4", 1, "k_render_flat<true,true,false,EVERY,1,false>", faithful=1),
    _row(RENDER, "S4", 3, "k_render_flat<false,true,true,EVERY,1,false>", count_work=1),
    _row(RENDER, "flat_mixed", 1, "k_render_flat<false,true,false,EVERY,1,false>", count_work=1),
    # ---------------------------------------------------------------- k_ss_frame_flat
    # more than 500,000 nodes: the 4K frame of test_gpu_parity.py::test_s5_4k_tile_sample_vs_oracle[1] is the launch that covers this one
    _row(SAMPLER, "S5", 1, "k_ss_frame_flat<false,TRI,5,true,false>", gpu=False),
    _row(SAMPLER, "S3small", 1, "k_ss_frame_flat<false,TRI,4,true,false>"),
    _row(SAMPLER, "mirror_tri", 1, "k_ss_frame_flat<false,TRI,1,false,false>"),
    _row(SAMPLER, "mirror_tri", 3, "k_ss_frame_flat<true,TRI,1,false,false>"),
    _row(SAMPLER, "materials", 3, "k_ss_frame_flat<true,EVERY,1,false,true>"),
    _row(SAMPLER, "S1", 1, "k_ss_frame_flat<false,EVERY,2,false,false>"),
    _row(SAMPLER, "S3mesh_small", 1, "k_ss_frame_flat<false,EVERY,2,false,false>"),
    _row(SAMPLER, "S1", 3, "k_ss_frame_flat<true,EVERY,2,false,false>"),
    _row(SAMPLER, "every_class", 3, "k_ss_frame_flat<true,EVERY,2,false,false>"),
    _row(SAMPLER, "mirror_mesh", 3, "k_ss_frame_flat<true,EVERY,2,false,false>"),
    _row(SAMPLER, "S4", 1, "k_ss_frame_flat<false,CSG|PRIMS,2,false,false>"),
    _row(SAMPLER, "S4", 3, "k_ss_frame_flat<true,CSG|PRIMS,2,false,false>"),
    # ---------------------------------------------------------------- k_trace_batch_flat: production, lean
    _row(TRACE, "S3small", 3, "k_trace_batch_flat<false,false,false,TRI,1>"),
    _row(TRACE, "S1", 1, "k_trace_batch_flat<false,false,false,SPHERE|PRIMS,1>"),
    _row(TRACE, "S3mesh_small", 1, "k_trace_batch_flat<false,false,false,MESH,1>"),
    _row(TRACE, "flat_mixed", 1, "k_trace_batch_flat<false,false,false,ALL,1>"),
    _row(TRACE, "every_class", 1, "k_trace_batch_flat<false,false,false,EVERY,2>"),
    _row(TRACE, "S4", 1, "k_trace_batch_flat<false,false,false,CSG|PRIMS,2>"),
    # ---------------------------------------------------------------- production, full
    _row(TRACE, "mirror_tri", 3, "k_trace_batch_flat<false,false,true,TRI,1>"),
    _row(TRACE, "S1", 3, "k_trace_batch_flat<false,false,true,SPHERE|PRIMS,1>"),
    _row(TRACE, "mirror_mesh", 3, "k_trace_batch_flat<false,false,true,MESH,1>"),
    _row(TRACE, "materials", 1, "k_trace_batch_flat<false,false,true,ALL,1>"),
    _row(TRACE, "every_class", 3, "k_trace_batch_flat<false,false,true,EVERY,2>"),
    _row(TRACE, "S4", 3, "k_trace_batch_flat<false,false,true,CSG|PRIMS,2>"),
    _row(TRACE, "quadrics", 3, "k_trace_batch_flat<false,false,true,CSG|PRIMS,2>"),
    # ---------------------------------------------------------------- faithful / counting
    _row(TRACE, "S1", 3, "k_trace_batch_flat<true,true,true,EVERY,1>", faithful=1),
    _row(TRACE, "S4", 1, "k_trace_batch_flat<true,true,false,EVERY,1>", faithful=1),
    _row(TRACE, "S4", 3, "k_trace_batch_flat<false,true,true,EVERY,1>", count_work=1),
    _row(TRACE, "flat_mixed", 1, "k_trace_batch_flat<false,true,false,EVERY,1>", count_work=1),
    # ---------------------------------------------------------------- the generic tier
    _row(RENDER, "nested", 3, "k_render_generic<lean>"),
    _row(RENDER, "nested", 3, "k_render_generic<counting>", count_work=1),
    _row(SAMPLER, "nested", 3, "k_ss_frame_generic<lean>"),
    _row(SAMPLER, "nested", 3, "k_ss_frame_generic<counting>", count_work=1),
    _row(TRACE, "nested", 3, "k_trace_batch_generic<lean>"),
    _row(TRACE, "nested", 3, "k_trace_batch_generic<counting>", count_work=1),
]
