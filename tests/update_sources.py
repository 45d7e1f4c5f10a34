"""What the tests of the fp32 and indexed update calls share (test_update_sources_host.py, test_update_sources_gpu.py) -- test
infrastructure beside bihs_refit.py, whose fixtures and poses these are.  The new calls are held to the fp64 calls on the WIDENED AND
GATHERED array, so a pose is rounded to fp32 and widened back first (r32): both calls then see the same doubles."""
import numpy as np

FAR = (4.0e4, -3.0e4, 5.0e4)            # far outside every fixture, well inside the reference's infinity (1e6): referenced by no item
NOT_A_NUMBER = (np.nan, np.nan, np.nan)  # referenced by no item either


def r32(a):
    """the array rounded to fp32 and widened back: what an fp32 producer holds, as doubles"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def pool(P, decoys=True, seed=31):
    """An n x 9 triangle array as a simulation would hold it: (verts [nv, 3] float64, idx [n, 3] int32) with verts[idx] == P to the bit.
    Every distinct vertex is held once, the pool is shuffled, and with `decoys` two vertices no item references lie among them: one far
    outside the scene, one NaN.  A bound folded over the vertex array instead of over the items would show either."""
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 9)
    bits = P.reshape(-1, 3).view(np.int64)  # (by bit pattern: -0.0 and 0.0 stay two vertices)
    uniq, inv = np.unique(bits, axis=0, return_inverse=True)
    held = uniq.view(np.float64).reshape(-1, 3)
    if decoys:
        held = np.concatenate([held, np.array([FAR, NOT_A_NUMBER])])
    slot = np.random.default_rng(seed).permutation(len(held))  # where entry j of `held` lies in the pool
    verts = np.empty_like(held)
    verts[slot] = held
    idx = np.ascontiguousarray(slot[np.asarray(inv).ravel()].reshape(-1, 3).astype(np.int32))
    assert verts[idx].reshape(-1, 9).tobytes() == P.tobytes()
    if decoys:
        assert not (set(slot[-2:].tolist()) & set(idx.ravel().tolist())) and len(P.reshape(-1, 3)) >= len(uniq)
    return verts, idx
