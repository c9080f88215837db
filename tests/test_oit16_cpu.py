"""Layered order-independent transparency of the native-storage build without a GPU: the emulated sequence -- the product's fp32 per-pixel bodies
(diligentfx_amd/csrc/mifx_oit.h) on the host, the inputs rounded to binary16 and the four targets rounded after the attenuation and after every colour draw
(tests/oit16_util.py emulate()) -- against the reference's outputs under the same rounding (tests/golden/oit16_golden.npz, written by
tests/golden/make_golden_oit16.py).  The bars are oit16_util's: layers and tail count exact, the transmittance by the contract, the targets within the contract's
allowance plus one binary16 spacing.  The device is held to the same emulation at the same bars by tests/h4_checks_shadows_oit.py."""
import numpy as np
import pytest

import oit16_util as U
import oit_util as O

F = np.float32


@pytest.fixture(scope="module")
def host_lib():
    lib = U.host_lib()
    if lib is None:
        pytest.skip("hipcc not available")
    return lib


@pytest.mark.parametrize("i,name", U.case_ids())
def test_the_emulated_sequence_against_the_reference_with_rgba16f_targets(host_lib, i, name):
    g = U.golden()
    c = O.cases()[i]
    assert str(g["names"][i]) == name == c["name"]
    got = U.emulate(host_lib, c, U.make_case16(c))
    U.check_against(got, (g[f"c{i}_layers"], g[f"c{i}_tail"], g[f"c{i}_targets"].astype(F)), name)


def test_fixture_is_not_the_fp32_one():
    """The rounding is visible: the inputs differ from oit_util's, and so do the expected targets and some layer words from tests/golden/oit_golden.npz's"""
    import os

    g, g32 = U.golden(), np.load(os.path.join(U.HERE, "golden", "oit_golden.npz"))
    cs = O.cases()
    assert [str(n) for n in g["names"]] == [c["name"] for c in cs]
    i = [c["name"] for c in cs].index("oit_67x35_k4_l7")
    d, d16 = O.make_case(cs[i]), U.make_case16(cs[i])
    assert not np.array_equal(d["base"], d16["base"]) and np.array_equal(d["depth"], d16["depth"]) and np.array_equal(d["alpha"], d16["alpha"])
    assert g[f"c{i}_targets"].dtype == np.float16 and not np.array_equal(g[f"c{i}_targets"].astype(F), U.q16(g32[f"c{i}_targets"]))
    assert not np.array_equal(g[f"c{i}_layers"], g32[f"c{i}_layers"])  # (the opacity is base_color.a, a binary16 value here)
    for j in range(len(cs)):
        assert float(g[f"c{j}_strict_vs_contracted"][0]) <= 0.5e-3 and float(g[f"c{j}_strict_vs_contracted"][1]) <= 1.0
