"""Golden G20: the state_dict schema of the REFERENCE's GnnNet(ResNet10), 5-way 5-shot, 84x84 -- key order, shapes and dtypes.

Build-container only (imports the reference through make_golden.import_reference).  Stores names, shapes and dtypes only, no
values: it is what tests/test_host_cpu.py::test_checkpoints_interchange_with_the_reference checks checkpoints against, so
the test runs without the reference.

    python oracle/make_golden_g20.py            # writes tests/golden/g20_reference_state_dict.npz
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402


def main():
    mods = MG.import_reference()
    ref = mods["methods.gnnnet"].GnnNet(MG.make_factory(mods["backbone"], 84), n_way=5, n_support=5)
    sd = ref.state_dict()
    nd = max(v.dim() for v in sd.values())
    shapes = np.full((len(sd), nd), -1, dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = v.shape
    out = os.path.join(MG.GOLD, "g20_reference_state_dict.npz")
    np.savez(out, keys=np.array(list(sd.keys())), shapes=shapes, ndim=np.array([v.dim() for v in sd.values()]),
             dtypes=np.array([str(v.dtype).replace("torch.", "") for v in sd.values()]))
    print("wrote", out, len(sd), "entries")


if __name__ == "__main__":
    main()
