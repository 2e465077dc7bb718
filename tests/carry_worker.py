"""Child process of tests/test_carry_gpu.py::test_rejected_corrections_in_a_child_process: the batch of that file with the carry on
and with NNMPC_CARRY=0 (read at every call), one handle each, under whatever environment the parent set (NNMPC_REFINE_TOL is read
once per process, hence a process of its own).  Leaves u, active, status and the counters of both runs in an .npz.

    python -m tests.carry_worker OUT.npz
"""
import os
import sys

import numpy as np


def main(path):
    from tests.test_carry_gpu import _batch, _call, _handle
    x0, lb, ub = _batch()
    res = {}
    for tag in ("on", "off"):
        if tag == "off":
            os.environ["NNMPC_CARRY"] = "0"
        qp = _handle()
        out = _call(qp, x0, lb, ub)
        qp.close()
        res.update({f"u_{tag}": out["u"], f"active_{tag}": out["active"], f"status_{tag}": out["status"],
                    f"carried_{tag}": out["stats"]["asm_carried"], f"rounds_{tag}": out["stats"]["asm_rounds"]})
    np.savez(path, **res)


if __name__ == "__main__":
    main(sys.argv[1])
