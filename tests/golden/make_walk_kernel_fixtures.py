"""Writes tests/golden/walk_kernel/{name}_{tile_bits}_{batch}.npy: <Z> of all 16 wires for the whole batch of the first
three cases of tests/test_gpu_walk_kernel.py, as the library of the checkout it is run in returns them -- taken once on
the GPU from a built checkout of the commit before k_measure_walk came in, where k_tile2 runs these walks, so that the
test can hold the new kernel's rows to k_tile2's bit for bit.

    cd BUILT_CHECKOUT_OF_THE_COMMIT_BEFORE && python THIS_TREE/tests/golden/make_walk_kernel_fixtures.py OUT_DIR

The package, the tapes and the angles (`_reference` of tests/test_gpu_measured_product_form.py) come from the checkout
in the working directory; OUT_DIR is tests/golden/walk_kernel of this tree.  [batch, 16] float32 each."""
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
CASES = (("all", 10, 160), ("all", 10, 640), ("all", 12, 640))


def main(out_dir):
    import torch

    from tests.test_gpu_measured_product_form import _reference
    from tests.test_measured_product_form_cpu import N_Q, plan_of

    os.makedirs(out_dir, exist_ok=True)
    for name, tile_bits, batch in CASES:
        struct, ang, _rows, _states = _reference(name, tile_bits, batch)
        plan = plan_of(struct, tile_bits)
        got = plan.run(torch.from_numpy(np.array(ang)).cuda(), "expval", list(range(N_Q))).cpu().numpy()
        last = plan.executed("expval").describe()["stages"][-1]
        assert last["last_group_lane_swap_last_run"] is True and last["staging_dma_last_run"] is True
        assert "walk_kernel_last_run" not in last, "run this in a checkout of the commit before"
        assert got.dtype == np.float32 and got.shape == (batch, N_Q)
        np.save(os.path.join(out_dir, "%s_%d_%d.npy" % (name, tile_bits, batch)), got)
        print(name, tile_bits, batch, got.shape, float(np.abs(got).max()))


if __name__ == "__main__":
    main(sys.argv[1])
