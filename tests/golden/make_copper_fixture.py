"""Generates tests/golden/copper_fixture.json: the RGB values of pbrt-v3's default metal, copper.

  python tests/golden/make_copper_fixture.py <pbrt-v3 source tree>

CreateMetalMaterial (src/materials/metal.cpp:112-121) defaults "eta" and "k" to RGBSpectrum::FromSampled(CopperWavelengths,
CopperN / CopperK, CopperSamples). FromSampled (src/core/spectrum.h:467-488) integrates the piecewise-linear spectrum
(InterpolateSpectrumSamples, spectrum.cpp:179-188) against the CIE matching functions (CIE_X / Y / Z at CIE_lambda,
spectrum.cpp) and converts with XYZToRGB (spectrum.h:56-60). This script reads those tables from the given source tree, replays
the arithmetic in float64 and writes the six results rounded to float32. The loader (loader_materials.cpp) carries them as constants;
tests/test_metal_substrate_scenes.py checks that the two agree. Nothing of the source tree is copied: the fixture holds six numbers.
"""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def read_array(text, name):
    m = re.search(r"const Float " + re.escape(name) + r"\[[^\]]*\]\s*=\s*\{(.*?)\};", text, re.S)
    if not m:
        raise SystemExit(f"array {name} not found")
    body = re.sub(r"//[^\n]*", "", m.group(1))
    return np.array([float(v.rstrip("fF")) for v in body.replace("\n", " ").split(",") if v.strip()], dtype=np.float64)


def interpolate(lam, vals, l):  # InterpolateSpectrumSamples, spectrum.cpp:179-188
    if l <= lam[0]:
        return vals[0]
    if l >= lam[-1]:
        return vals[-1]
    off = int(np.searchsorted(lam, l, side="right")) - 1  # FindInterval: the last index with lam[index] <= l
    off = min(max(off, 0), len(lam) - 2)
    t = (l - lam[off]) / (lam[off + 1] - lam[off])
    return (1 - t) * vals[off] + t * vals[off + 1]  # Lerp


def from_sampled(lam, vals, cie_lambda, cx, cy, cz, y_integral):  # RGBSpectrum::FromSampled, spectrum.h:467-488
    assert np.all(np.diff(lam) > 0)
    xyz = np.zeros(3)
    for i in range(len(cie_lambda)):
        v = interpolate(lam, vals, cie_lambda[i])
        xyz += v * np.array([cx[i], cy[i], cz[i]])
    xyz *= (cie_lambda[-1] - cie_lambda[0]) / (y_integral * len(cie_lambda))
    x, y, z = xyz  # XYZToRGB, spectrum.h:56-60
    return [3.240479 * x - 1.537150 * y - 0.498535 * z,
            -0.969256 * x + 1.875991 * y + 0.041556 * z,
            0.055648 * x - 0.204043 * y + 1.057311 * z]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    src = os.path.join(sys.argv[1], "src")
    metal = open(os.path.join(src, "materials", "metal.cpp")).read()
    spectrum = open(os.path.join(src, "core", "spectrum.cpp")).read()
    header = open(os.path.join(src, "core", "spectrum.h")).read()
    y_integral = float(re.search(r"CIE_Y_integral\s*=\s*([0-9.eE+-]+)", header).group(1))
    cie = [read_array(spectrum, n) for n in ("CIE_lambda", "CIE_X", "CIE_Y", "CIE_Z")]
    lam = read_array(metal, "CopperWavelengths")
    out = {}
    for key, name in (("eta", "CopperN"), ("k", "CopperK")):
        rgb = from_sampled(lam, read_array(metal, name), *cie, y_integral)
        out[key] = [float(np.float32(v)) for v in rgb]
    path = os.path.join(HERE, "copper_fixture.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path, out)


if __name__ == "__main__":
    main()
