"""GPU (-m gpu): the seeded random shapes of tests/fuzz_added_ops.py for `filter2d`, `composite_layers`, `shade`,
`mesh_laplacian` / `cotangent_weights` and `msi` -- five operators that were tested on fixed shape lists only -- through the
C ABI binding and the Python API, against their oracles under the bounds of their own test modules."""
import pytest

import fuzz_added_ops as F

pytestmark = pytest.mark.gpu
PER_BLOCK, BLOCKS = 40, 6


@pytest.mark.parametrize("block", range(BLOCKS))
def test_randomised_shapes(block):
    """40 seeded cases per block.  What the 240 seeds hold -- every operator at least 35 times, over 80 generic filter2d
    triples, incidence rows of exactly 256, 257, 512 and 513 entries, msi textures one texel high and one texel wide, every
    option, layout and form of shade and composite_layers -- tests/test_fuzz_added_ops_host.py counts on the CPU."""
    for seed in range(PER_BLOCK * block, PER_BLOCK * (block + 1)):
        c = F.make_case(seed)
        try:
            F.run_case(c)
        except AssertionError as e:
            raise AssertionError(f"{F.describe(c)}: {e}") from e
