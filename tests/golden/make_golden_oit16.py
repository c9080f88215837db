#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/oit16_golden.npz: what the REFERENCE's layered order-independent transparency makes of the cases of
tests/oit_util.py when its four targets are RGBA16_FLOAT, as the reference's are -- the expectation of the native-storage build of the library.

Run by hand where the reference tree is mounted (MIFX_REFERENCE_ROOT, default /root/reference); never by build(), smoke(), bench.py or a test:

    python tests/golden/make_golden_oit16.py

The units and prepare() are make_golden_oit.py's, as they are (they #include the reference's files by name at generation time and hold none of their text); the
cases are tests/oit_util.py's.  What differs from make_golden_oit.py:
  * every 4-channel input (a slice's base colour, material, radiance and specular IBL, and the four targets) is rounded to binary16 first (tests/oit16_util.py
    make_case16): the values an RGBA16_FLOAT plane can hold; depth, colour alpha and the opaque depth stay fp32;
  * the four targets are rounded to binary16 after the attenuation and after every ref_oit_blend call: a blend is evaluated in fp32 and its store rounds.
The targets are stored as float16.  Every case is built twice (strict fp32, and -ffp-contract=fast -march=native): the layers and the tail's count must be equal;
the largest difference of the tail's transmittance (util.assert_close's measure) and of the targets (in binary16 steps) is stored."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import make_golden_grid as MG  # noqa: E402
import make_golden_oit as MO  # noqa: E402
import oit16_util as U  # noqa: E402
import oit_util as O  # noqa: E402
import util  # noqa: E402

F = np.float32


def run_case16(lib, c, d):
    """make_golden_oit.run_case with the targets rounded to binary16 after the attenuation and after every colour draw"""
    w, h, k, n = c["w"], c["h"], c["k"], c["l"]
    up, fp = MO.up, MO.fp
    cam = np.ascontiguousarray(d["camera"], F).tobytes()
    layers = np.full((h, w, k), 0xDEADBEEF, np.uint32)
    assert lib.ref_oit_clear(up(layers), cam, w, h, k) == 576
    tail = np.zeros((h, w, 4), F)
    tail[..., 3] = 1
    for i in range(n):
        assert lib.ref_oit_update(up(layers), fp(tail), fp(d["depth"][i]), fp(d["base"][i]), fp(d["opaque"]), cam, w, h, k) == 576
    t = [np.ascontiguousarray(d["targets"][j]).copy() for j in range(4)]
    assert lib.ref_oit_attenuate(up(layers), fp(tail), fp(t[0]), fp(t[1]), fp(t[2]), fp(t[3]), cam, w, h, k) == 576
    t = [np.ascontiguousarray(U.q16(a)) for a in t]
    for i in range(n):
        alpha = None if d["alpha"] is None else d["alpha"][i]
        assert lib.ref_oit_blend(up(layers), fp(tail), fp(d["depth"][i]), fp(d["base"][i]), fp(d["material"][i]), fp(d["radiance"][i]), fp(d["ibl"][i]), fp(alpha), fp(d["opaque"]),
                                 fp(t[0]), fp(t[1]), fp(t[2]), fp(t[3]), cam, w, h, k) == 576
        t = [np.ascontiguousarray(U.q16(a)) for a in t]
    return layers, np.ascontiguousarray(tail[..., [0, 3]]), np.stack(t)


def main():
    assert os.path.isdir(os.path.join(MG.REFERENCE_ROOT, "Shaders")), "the reference tree is not mounted"
    cs = O.cases()
    fx = {"names": np.array([c["name"] for c in cs])}
    with tempfile.TemporaryDirectory(prefix="mifx_oit16_golden_") as tmp:
        MO.prepare(tmp)
        strict, fast = MG.build(MO.UNITS, MG.STRICT, tmp, "strict"), MG.build(MO.UNITS, MG.CONTRACTED, tmp, "fast")
        for i, c in enumerate(cs):
            d = U.make_case16(c)
            (la, ta, ga), (lb, tb, gb) = run_case16(strict, c, d), run_case16(fast, c, d)
            assert np.isfinite(ta).all() and np.isfinite(ga).all(), c["name"]
            assert np.array_equal(la, lb) and np.array_equal(ta[..., 0], tb[..., 0]), f"{c['name']}: the layers or the tail count differ between the reference's own builds"
            diff = float(util.rel_err(tb[..., 1], ta[..., 1]).max())
            steps = float((np.abs(ga.astype(np.float64) - gb) / np.abs(np.spacing(ga.astype(np.float16))).astype(np.float64)).max())
            print(f"{c['name']:28s} layers in use {int((la != 0xFFFFFFFF).sum()):6d}  tail pixels {int((ta[..., 0] > 0).sum()):5d}  texels changed {int((ga != d['targets']).any(-1).sum()):6d}  "
                  f"strict vs contracted: transmittance max rel {diff:.3e}, targets at most {steps:.2f} binary16 steps apart")
            assert diff <= 0.5e-3 and steps <= 1.0, f"{c['name']}: the reference's own two builds differ -- change the case"
            q = f"c{i}_"
            fx[q + "layers"], fx[q + "tail"], fx[q + "targets"], fx[q + "strict_vs_contracted"] = la, ta, ga.astype(np.float16), np.array([diff, steps])
            assert np.array_equal(fx[q + "targets"].astype(F), ga)
    path = os.path.join(HERE, "oit16_golden.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200_000


if __name__ == "__main__":
    main()
