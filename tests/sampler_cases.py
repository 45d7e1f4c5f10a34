"""The cases on which the adaptive sampler is held to tests/sampler_model.py, bit for bit: by the host build
(test_sampler_model_host.py, which also asserts what the table as a whole reaches) and by the GPU (test_sampler_model_gpu.py).

A case is (scene, W, H, maxdepth, blocksize, thresholds, frames per launch).  Frames are small -- the largest is 130x131 -- and
chosen for the tile shapes they leave: chunk(W, blocksize) gives the tile widths, the last the remainder, so 66 = 65 + 1,
67 = 65 + 2, 131 = 65 + 65 + 1 and 130 = 65 + 65.  Every case must keep all its contrasts at least four bands (sampler_model.BAND)
from its thresholds on the host build's samples; where a frame did not, its size or its thresholds were changed, never the band."""
from collections import namedtuple

import zoo
from glome_amd import api, scenes

Case = namedtuple("Case", "scene w h maxdepth blocksize thresholds nframes note")

SCENES = {"S1": lambda: scenes.s1(nlights=2), "S3small": lambda: scenes.s3(24), "S4": scenes.s4, "materials": zoo.materials,
          "mesh": zoo.mesh_scene, "nested": zoo.nested}
GENERIC = ("nested",)  # the scenes of the generic tier (its own sampler kernel); the others are flat-tier scenes

# Thresholds other than the default.  Each set sits in a gap of its case's contrasts (found pass by pass on the host build: the
# widest gap near the value aimed at), since a frame with a few thousand candidates per pass -- a batch has that many per view --
# seldom leaves four bands free around a value picked beforehand.
OTHER_THRESHOLDS = (0.11, 0.1884, 0.116, 0.2799)
S4_BATCH_THRESHOLDS = (0.14, 0.1428, 0.1658, 0.1828)
NESTED_BATCH_THRESHOLDS = (0.1019, 0.1827, 0.1568, 0.1742)

CASES = [
    # ---- one frame per launch (flat tier: region size 0; generic tier: 1x1 blocks)
    Case("S1", 71, 71, 3, 65, None, 1, "tiles clipped on the right, at the bottom and at both"),
    Case("S3small", 131, 66, 3, 65, None, 1, "the hand-written triangle walk; last tile column 1 pixel wide, last tile row 1 pixel high"),
    Case("materials", 67, 40, 3, 65, None, 1, "secondary rays; last tile column 2 pixels wide"),
    Case("S4", 70, 33, 3, 16, None, 1, "CSG | PRIMS; blocksize 16"),
    Case("mesh", 66, 70, 3, 65, None, 1, "last tile column 1 pixel wide"),
    Case("materials", 50, 37, 3, 7, None, 1, "blocksize 7"),
    Case("nested", 70, 45, 3, 65, None, 1, "the generic tier's sampler"),
    Case("nested", 33, 64, 3, 16, None, 1, "the generic tier's sampler, blocksize 16, last tile column 1 pixel wide"),
    Case("S1", 1, 1, 3, 65, None, 1, "a 1x1 frame"),
    Case("S3small", 7, 5, 3, 65, None, 1, "smaller than a block of any pass"),
    Case("S4", 65, 65, 3, 65, None, 1, "one full tile"),
    Case("S3small", 130, 131, 1, 65, None, 1, "2x2 full tiles side by side (lean shading), and a row of tiles 1 pixel high"),
    Case("S1", 9, 6, 3, 1, None, 1, "blocksize 1: every pixel a tile of its own"),
    Case("materials", 67, 40, 3, 65, OTHER_THRESHOLDS, 1, "thresholds other than the default"),
    Case("S4", 40, 23, 3, 16, OTHER_THRESHOLDS, 1, "thresholds other than the default, blocksize 16"),
    # ---- several frames per launch: the region shape follows them (flat: sizes 0, 1, 2; generic: 2x1 from pass 3, the twelve-frame table)
    Case("S3small", 72, 66, 1, 65, None, 2, "flat tier, region size 0"),
    Case("S3small", 72, 66, 1, 65, None, 3, "flat tier, region size 1"),
    Case("S3small", 72, 66, 1, 65, None, 8, "flat tier, region size 2"),
    Case("S4", 50, 37, 3, 16, S4_BATCH_THRESHOLDS, 8, "flat tier, region size 2, blocksize 16"),
    Case("nested", 36, 67, 3, 65, NESTED_BATCH_THRESHOLDS, 3, "generic tier, 2x1 blocks from pass 3"),
    Case("nested", 36, 67, 3, 65, NESTED_BATCH_THRESHOLDS, 12, "generic tier, the twelve-frame table"),
]


def case_id(c):
    t = "" if c.thresholds is None else "-thr"
    return f"{c.scene}-{c.w}x{c.h}-md{c.maxdepth}-bs{c.blocksize}{t}-n{c.nframes}"


SINGLE = [c for c in CASES if c.nframes == 1]
BATCH = [c for c in CASES if c.nframes > 1]


def views(c, sd):
    """The cameras of a case's launch: the scene's own, then the eye moved sideways and up a little per frame."""
    pos, at, up, angle = sd.cam
    return [api.camera([pos[0] + 0.4 * f, pos[1] + 0.1 * f, pos[2]], at, up, angle) for f in range(c.nframes)]
