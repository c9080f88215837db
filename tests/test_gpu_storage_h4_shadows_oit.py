"""The cascaded shadow maps and the layered order-independent transparency in the native-storage build of the library (libmifx_h4.so).  The storage mode is a
property of the loaded library, so the checks run in a process of their own (tests/h4_checks_shadows_oit.py) with MIFX_STORAGE=h4, as tests/test_gpu_storage_h4.py
runs the chain's."""
import os
import subprocess
import sys

import pytest

from util import ROOT


@pytest.mark.gpu
@pytest.mark.parametrize("section", ["shadows", "oit"])
def test_shadows_and_oit_in_the_native_storage_build(section):
    """shadows: conversion and look-up cases of the 32-bit fixture, and every check of the 16-bit filterable formats; oit: every case by the sequence and by the fused
    entries, bit for bit the same, against the emulated expectation and the reference fixture with RGBA16_FLOAT targets"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "h4_checks_shadows_oit.py"), section], cwd=ROOT, env=dict(os.environ, MIFX_STORAGE="h4"), capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "h4 checks OK" in r.stdout and f"h4 section {section} OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
