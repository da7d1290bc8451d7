"""The ray scan backward at its tile edges.  csrc/rdrf_bwd_mlp_dev.hpp has the scan as functions of the group width (scan_sample,
tile_carries, suffix_g_alpha, dist_grads): 32 wide for the dynamic field (k_ray_scan_bwd on the flat path, 16 rays per workgroup;
k_dyn_density_bwd<0> per ray); the static field's k_static_density_bwd runs the same lines 64 wide.  The z_vals gradient test reaches every
term of it -- d(weight), d(sigma), d(dists) and the g_z updates of both fields -- so it runs here with S on either side of
the 32- and 64-sample tile edges and N on either side of 16 rays, against the oracle's autograd at that test's tolerances."""
import pytest

from test_gpu_backward import z_vals_gradient_check

pytestmark = pytest.mark.gpu

# (N, S): one sample pair; below / at / above one 32-sample tile; below / at / above one 64-sample tile; five 32-sample tiles
SHAPES = [(1, 2), (17, 31), (16, 32), (17, 33), (1, 63), (16, 64), (17, 65), (3, 129)]
# ray seed of a case (default: the seed of test_z_vals_gradient_matches_oracle).  A case whose input sits on a ReLU kink with
# the default seed -- it then fails against the library of the commit before this file too -- gets another seed here
RAY_SEED = {}


@pytest.mark.parametrize("N,S", SHAPES)
@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_z_vals_gradient_at_the_scan_tile_edges(rt, N, S):
    z_vals_gradient_check(rt, N, S, RAY_SEED.get((rt, N, S), 21))
