"""GPU suite (-m gpu): every separately compiled render, sampler and trace kernel is launched and compared with the oracle -- one case per
row of tests/instance_ledger.py (tests/test_instance_ledger.py asserts, without a GPU, that the rows name every instance and that each
row's launch gets the instance it names).

Per row: the launch with the row's parameters against the fp64 oracle under the gates of tests/parity.py as they are (check_image for
render and trace rows, check_subsample_image for sampler rows; ray counts as those check them); the same launch a second time, bit for
bit; and, for a flat-tier row that asks for neither `faithful` nor `count_work`, the same launch with faithful=1 and with count_work=1 --
other instances of the same source, which must give the same bits and the same ray counts (glome_amd/build.py: contraction is decided
per source expression so that every instance rounds identically).

With GLOME_PARITY_LOG set, parity._log writes each row's levels under the row's id."""
import numpy as np
import pytest

import instance_ledger as ledger
import parity
from helpers import product_camera_lights
from glome_amd import api

pytestmark = pytest.mark.gpu

ROWS = [r for r in ledger.LAUNCHES if r.gpu]
RAY_KEYS = ("rays_primary", "rays_shadow", "rays_secondary")


class Committed:
    def __init__(self, ctx, make):
        self.sd = make()
        self.b = api.Builder()
        self.nm, _ = self.sd.replay(self.b)
        self.sc = ctx.commit(self.b, self.nm[self.sd.root])
        self.cam, self.lights = product_camera_lights(self.sd)


@pytest.fixture(scope="module")
def committed(gpu_ctx):
    """a row's scene on the GPU, committed once per module"""
    cache = {}

    def get(row):
        if row.make not in cache:
            cache[row.make] = Committed(gpu_ctx, row.make)
        return cache[row.make]
    yield get
    for c in cache.values():
        c.sc.release()


def launch(c, row, faithful, count_work):
    """-> (frame [h, w, 5] float32, ray counts) of the row's launch with the two flags as given"""
    if row.kind == ledger.TRACE:
        o, d = api.frame_rays(c.cam, row.width, row.height)
        r = c.sc.trace(o, d, c.lights, params=api.trace_params(maxdepth=row.maxdepth, faithful=faithful, count_work=count_work))
        st = r["stats"]
        assert st["n_pixels"] == row.width * row.height
        img = np.concatenate([r["rgba"], r["depth"][:, None]], axis=1).reshape(row.height, row.width, 5)
    else:
        P = api.render_params(width=row.width, height=row.height, mode=1 if row.kind == ledger.SAMPLER else 0, maxdepth=row.maxdepth, faithful=faithful, count_work=count_work)
        img, _, st = c.sc.render(c.cam, c.lights, P, want_packed=False)
    return np.ascontiguousarray(img), [st[k] for k in RAY_KEYS]


def differing(a, b):
    bad = np.flatnonzero(np.any(a.view(np.uint32) != b.view(np.uint32), axis=-1))
    return len(bad), bad[:8].tolist()


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_instance_against_the_oracle_and_the_other_instances(committed, row):
    c = committed(row)
    assert c.sc.info()["tier"] == (1 if "_generic<" in row.instance else 0)
    img, counts = launch(c, row, row.faithful, row.count_work)
    c.sd.name = row.id + " " + row.instance  # (what parity._log names the levels by)
    if row.kind == ledger.SAMPLER:
        parity.check_subsample_image(img, counts, c.sd, row.width, row.height, row.maxdepth)
    else:
        parity.check_image(img, counts, c.sd, row.width, row.height, row.maxdepth)
    # a second run of the same launch: the same bits, whatever order the work queue was served in
    again, counts2 = launch(c, row, row.faithful, row.count_work)
    assert np.array_equal(img.view(np.uint32), again.view(np.uint32)) and counts == counts2, ("second run", differing(img, again), counts, counts2)
    # the faithful and the counting instance give the frame of the early-out one
    if "_flat<" in row.instance and not row.faithful and not row.count_work:
        for what, f, cw in (("faithful", 1, 0), ("count_work", 0, 1)):
            other, ocounts = launch(c, row, f, cw)
            same = np.array_equal(img.view(np.uint32), other.view(np.uint32))
            parity._log("bit_identity_" + what, c.sd, {"identical": bool(same), "differing_pixels": differing(img, other)[0], "counts": counts, "other_counts": ocounts})
            assert same, (what, "pixels that differ", differing(img, other))
            assert counts == ocounts, (what, counts, ocounts)
