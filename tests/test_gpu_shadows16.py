"""The 16-bit filterable shadow maps on the GPU, in the fp32 library: RG16_UNORM (VSM), RG16_FLOAT (EVSM2) and RGBA16_FLOAT (EVSM4) through the C ABI against the
reference fixture (tests/golden/shadows16_golden.npz), the fused conversion against the two launches bit for bit, pitched outputs whose poisoned padding stays
untouched, the look-ups from the fixture's maps, the refusals with a context, and the Python mirror end to end.

Shapes (the fixture's): 13x9x1 with iFixedFilterSize 2, 3 and 7 -- the halo lies outside the slice on every side; 50x38x3 with the two world-radius sets, one inside
the fused kernel's range and one beyond it; 260x70x2 -- five tiles across, a width that is no multiple of 64.  Look-ups at 67x45, 2x2 and 1x1.

Bars (shadows16_util): conversion codes within one step of the format on top of util.assert_close's defaults, no outliers; look-ups within the fixture's stored
budgets (all zero: the project's contract), the cascade index exact.  The checks themselves are shadows16_checks', which tests/h4_checks_shadows_oit.py runs again in
the native-storage library."""
import pytest

import shadows16_checks as K
import shadows16_util as U
from util import blue_noise_tables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from diligentfx_amd import api

    sobol, tile = blue_noise_tables()
    return api.PostFXContext(0, sobol, tile)


@pytest.fixture(scope="module")
def host_lib():
    lib = U.host_lib()
    assert lib is not None, "hipcc not available: the host harness, which the Python mirror's look-up is compared with, cannot be built"
    return lib


@pytest.mark.parametrize("i,name", U.conv_cases())
def test_conversion_codes_fused_and_two_launch_on_pitched_poisoned_arrays(mifx_lib, ctx, i, name):
    K.check_conversion_case(ctx, i, name)


@pytest.mark.parametrize("i,name", U.look_cases())
def test_lookup_from_the_fixtures_16bit_maps(mifx_lib, ctx, i, name):
    K.check_lookup_case(ctx, i, name)


def test_refusals_through_the_entries_with_a_context(mifx_lib, ctx):
    K.check_refusals_with_a_context(ctx)


def test_python_mirror_keeps_the_callers_flag_for_fp32_maps(mifx_lib, ctx):
    K.check_python_mirror_keeps_the_callers_flag_for_fp32_maps(ctx)


@pytest.mark.parametrize("mode", [2, 3, 4])
def test_python_mirror_convert_then_filter_end_to_end(mifx_lib, ctx, host_lib, mode):
    K.check_python_mirror(ctx, host_lib, mode)
