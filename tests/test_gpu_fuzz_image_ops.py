"""GPU (-m gpu): the seeded random shapes of tests/fuzz_image_ops.py for `ssim`, `photometric_loss` and `mipmap_pyramid` --
the two operators that were tested on fixed shape lists only -- through the C ABI binding and the Python API, against their
oracles under the bounds of their own test modules."""
import pytest

import fuzz_image_ops as F

pytestmark = pytest.mark.gpu
PER_BLOCK, BLOCKS = 48, 5


@pytest.mark.parametrize("block", range(BLOCKS))
def test_randomised_shapes(block):
    """48 seeded cases per block.  The 240 seeds hold each of the four operators at least 50 times, every weight kind, layout,
    padding, window and precision, seven means over more than 256 views, 60 maps of three tiles or more across and seven
    "valid" maps with an interior tile (tests/test_image_loss_host.py counts them)."""
    for seed in range(PER_BLOCK * block, PER_BLOCK * (block + 1)):
        c = F.make_case(seed)
        try:
            F.run_case(c)
        except AssertionError as e:
            raise AssertionError(f"{F.describe(c)}: {e}") from e
