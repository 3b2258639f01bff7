"""Writes host_loop_vectors.npz: moment vectors of short ICP loops whose count is the same in every pass, and what
icp_host_loop_advance / icp_host_loop_state made of them -- recorded from the build of the commit BEFORE the batch gate changed the
error's divisor to the count of the previous vector.  tests/test_batch_gate_abi.py feeds the vectors to the current build and
compares bytes.  To regenerate (only ever against that older build):

    ICP_LIB_PATH=/path/to/older/libicp_mi355x.so python tests/golden/make_host_loop_vectors.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_moments as rm                      # noqa: E402
import ref_numpy                              # noqa: E402
from clouds import ragged_pair                # noqa: E402
from __graft_entry__ import load_package      # noqa: E402

CASES = {   # name: (plane, dtype, max_iter, tol, fixed)
    "p2p_f32_fixed": (False, np.float32, 5, 0.0, True),
    "p2p_f64_stop": (False, np.float64, 12, 1e-4, False),
    "plane_f32_fixed": (True, np.float32, 4, 0.0, True),
    "plane_f64_stop": (True, np.float64, 12, 1e-4, False),
}


def vectors(pkg, name):
    plane, dtype, max_iter, tol, fixed = CASES[name]
    D, M = (a.astype(dtype) for a in ragged_pair(200300, 200, 300))
    rng = np.random.default_rng(5)
    N = rng.standard_normal(M.shape)
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(dtype)
    loop = pkg.distributed.HostLoop(metric=pkg.ICP_POINT_TO_PLANE if plane else pkg.ICP_POINT_TO_POINT, max_iter=max_iter, tol=tol,
                                    fixed_iterations=fixed, precision=pkg.ICP_F64 if dtype == np.float64 else pkg.ICP_F32)
    P, idx_prev, out = D, None, dict(mom=[], done=[], R=[], t=[])
    for k in range(max_iter + 1):
        final = k == max_iter
        idx = ref_numpy.nn(P, M)
        terms = rm.plane_point_terms(P, M, N, idx, idx_prev) if plane else rm.p2p_point_terms(P, M, idx, idx_prev)
        mom = terms.sum(axis=0)
        if final:   # the loop's last pass carries the error alone
            mom[1:] = 0.0
        done, R, t = loop.advance(mom)
        out["mom"].append(mom)
        out["done"].append(done)
        out["R"].append(R.reshape(9).copy())
        out["t"].append(t.copy())
        if done:
            break
        loop.note_applied()
        P, idx_prev = rm.apply_rt(P, R, t), idx
    st = loop.state()
    res = {f"{name}.{k}": np.array(v) for k, v in out.items()}
    res.update({f"{name}.err": st["err"], f"{name}.T": st["T"], f"{name}.iterations": np.int32(st["iterations"]),
                f"{name}.passes": np.int32(st["passes"])})
    return res


if __name__ == "__main__":
    pkg = load_package()
    data = {}
    for name in CASES:
        data.update(vectors(pkg, name))
    np.savez(os.path.join(HERE, "host_loop_vectors.npz"), **data)
    print({k: v.shape for k, v in data.items()})
