"""GPU (-m gpu): the seeded random cases of tests/fuzz_geometry.py for `face_info`, `vert_normals`, `face_attribute_to_vert`,
`face_dpdt` and `vert_binormals` -- UV topologies of their own, incidence rows that end in a partial chunk, lane counts one
either side of a block -- through the Python API and the C ABI binding, against the PyTorch formulation on the CPU under the
bounds of tests/test_gpu_geometry.py."""
import pytest

import fuzz_geometry as F

pytestmark = pytest.mark.gpu
PER_BLOCK, BLOCKS = 40, 6


@pytest.mark.parametrize("block", range(BLOCKS))
def test_randomised_meshes(block):
    """40 seeded cases per block.  What the 240 seeds hold -- every UV topology at least 30 times, `few` with a UV row of more
    than a chunk at least 20 times, fans of valence 255, 256, 257, 300, 511, 512 and 513, chunked rows with A = 1, 2, 5 and 9,
    N F and N V on 255, 256, 257, 511, 512 and 513, a face list per view at least 30 times -- and that every draw meets the
    conditions its bounds rest on, tests/test_fuzz_geometry_host.py shows on the CPU."""
    for seed in range(PER_BLOCK * block, PER_BLOCK * (block + 1)):
        c = F.make_case(seed)
        try:
            F.run_case(c)
        except AssertionError as e:
            raise AssertionError(f"{F.describe(c)}: {e}") from e
