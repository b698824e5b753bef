"""m_sign (csrc/physics.h) against the definition it replaced, and sincos2x2 (csrc/stage_f32.h) against two
sincos2 calls, bitwise, on the host.

A small stand-alone host program includes stage_f32.h, reads bit patterns and writes
 * m_sign of each beside (R)((x > 0) - (x < 0)), the former definition, for float and double; once in the default
   floating-point mode and once with denormal inputs read as zero (the x86 DAZ / FTZ bits: what the kernels'
   flush-to-zero mode does to the two compares).  Inputs: +-0, the smallest and largest denormals, +-1, +-inf,
   NaNs of both signs, and 10^6 random bit patterns;
 * sincos2x2({a, b}) beside (sincos2(a), sincos2(b)).  Inputs: a grid over +-4 pi, huge arguments (1e8, 1e30),
   NaN and inf, and 10^6 random pairs (half of them random bit patterns, half uniform in +-4 pi)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SRC = r"""
#include "stage_f32.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <xmmintrin.h>
template <typename R> static R sign_former(R x) { return (R)((x > (R)0) - (x < (R)0)); }
template <typename R> static int run(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    const size_t n = (size_t)bytes / sizeof(R);
    R* x = (R*)malloc(n * sizeof(R));
    R* y = (R*)malloc(2 * n * sizeof(R));
    if (fread(x, sizeof(R), n, f) != n) return 3;
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        volatile R v = x[i];
        y[i] = hg::m_sign((R)v);
        y[n + i] = sign_former<R>((R)v);
    }
    f = fopen(out, "wb");
    if (!f || fwrite(y, sizeof(R), 2 * n, f) != 2 * n) return 4;
    fclose(f);
    free(x);
    free(y);
    return 0;
}
// pairs (a, b) in: per pair sincos2x2's four floats, then sincos2(a)'s and sincos2(b)'s
static int run_sincos(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const size_t n = (size_t)ftell(f) / (2 * sizeof(float));
    fseek(f, 0, SEEK_SET);
    float* x = (float*)malloc(2 * n * sizeof(float));
    float* y = (float*)malloc(8 * n * sizeof(float));
    if (fread(x, 2 * sizeof(float), n, f) != n) return 3;
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        volatile float a = x[2 * i], b = x[2 * i + 1];
        const hg::SinCos2 w = hg::sincos2x2(hg::f2{a, b});
        const hg::f2 p = hg::sincos2(a), q = hg::sincos2(b);
        float* o = y + 8 * i;
        o[0] = w.a.x; o[1] = w.a.y; o[2] = w.b.x; o[3] = w.b.y;
        o[4] = p.x; o[5] = p.y; o[6] = q.x; o[7] = q.y;
    }
    f = fopen(out, "wb");
    if (!f || fwrite(y, 8 * sizeof(float), n, f) != n) return 4;
    fclose(f);
    free(x);
    free(y);
    return 0;
}
int main(int argc, char** argv) {
    if (argc != 5) return 1;
    if (atoi(argv[2])) _mm_setcsr(_mm_getcsr() | 0x8040);   // FTZ | DAZ
    if (strcmp(argv[1], "sincos") == 0) return run_sincos(argv[3], argv[4]);
    return strcmp(argv[1], "f32") == 0 ? run<float>(argv[3], argv[4]) : run<double>(argv[3], argv[4]);
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("sign_host")
    src = d / "sign_host.cpp"
    src.write_text(SRC)
    exe = d / "sign_host"
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=on",
                           "-I", os.path.join(ROOT, "heli-gym_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)])
    return d, exe


def _inputs(ftype, utype):
    info = np.finfo(ftype)
    nbits = info.bits
    sign = utype(1) << utype(nbits - 1)
    mant = (utype(1) << utype(info.nmant)) - utype(1)
    expo = (sign - utype(1)) & ~mant
    pos = [utype(0), utype(1), mant, np.array(1, ftype).view(utype)[()], expo,   # 0, denormal min / max, 1, inf
           expo | (utype(1) << utype(info.nmant - 1)), expo | utype(1)]          # quiet NaN, signalling NaN
    special = np.array(pos + [p | sign for p in pos], dtype=utype)
    rng = np.random.default_rng(20261020)
    rand = rng.integers(0, np.iinfo(utype).max, size=10 ** 6, dtype=utype, endpoint=True)
    return np.concatenate([special, rand])


@pytest.mark.parametrize("daz", [0, 1], ids=["ieee", "flush"])
@pytest.mark.parametrize("name,ftype,utype", [("f32", np.float32, np.uint32), ("f64", np.float64, np.uint64)])
def test_m_sign_equals_former_definition_bitwise(prog, name, ftype, utype, daz):
    d, exe = prog
    x = _inputs(ftype, utype)
    fin, fout = d / f"{name}_{daz}.in", d / f"{name}_{daz}.out"
    x.tofile(fin)
    subprocess.check_call([str(exe), name, str(daz), str(fin), str(fout)], timeout=120)
    y = np.fromfile(fout, dtype=utype).reshape(2, -1)
    assert y.shape[1] == x.size
    bad = np.nonzero(y[0] != y[1])[0]
    assert bad.size == 0, [(hex(int(x[i])), hex(int(y[0, i])), hex(int(y[1, i]))) for i in bad[:8]]
    # and the values are the three the reward can take: +1, -1, +0
    one = np.array(1, ftype).view(utype)[()]
    assert set(np.unique(y[0]).tolist()) <= {0, int(one), int(one | (utype(1) << utype(np.finfo(ftype).bits - 1)))}


@pytest.mark.parametrize("daz", [0, 1], ids=["ieee", "flush"])
def test_sincos2x2_equals_two_sincos2_bitwise(prog, daz):
    d, exe = prog
    rng = np.random.default_rng(4)
    grid = np.linspace(-4 * np.pi, 4 * np.pi, 4097).astype(np.float32)
    odd = np.array([0.0, -0.0, 1e8, -1e8, 1e30, -1e30, np.nan, -np.nan, np.inf, -np.inf, 1e-40, -1e-40,
                    np.pi / 4, np.pi / 2, np.pi, 3.14159274], dtype=np.float32)
    a = np.concatenate([grid, grid, odd, np.repeat(odd, odd.size),
                        rng.integers(0, 2 ** 32, size=500_000, dtype=np.uint32).view(np.float32),
                        rng.uniform(-4 * np.pi, 4 * np.pi, 500_000).astype(np.float32)])
    b = np.concatenate([grid[::-1], np.roll(grid, 1234), odd[::-1], np.tile(odd, odd.size),
                        rng.integers(0, 2 ** 32, size=500_000, dtype=np.uint32).view(np.float32),
                        rng.uniform(-4 * np.pi, 4 * np.pi, 500_000).astype(np.float32)])
    assert a.size == b.size >= 10 ** 6
    fin, fout = d / f"sincos_{daz}.in", d / f"sincos_{daz}.out"
    np.stack([a, b], axis=1).astype(np.float32).tofile(fin)
    subprocess.check_call([str(exe), "sincos", str(daz), str(fin), str(fout)], timeout=120)
    y = np.fromfile(fout, dtype=np.uint32).reshape(-1, 2, 4)
    assert y.shape[0] == a.size
    bad = np.nonzero((y[:, 0] != y[:, 1]).any(axis=1))[0]
    assert bad.size == 0, [(float(a[i]), float(b[i]), y[i].tolist()) for i in bad[:8]]
    # (the comparison is of something: a finite pair's results are sin / cos to a few ulps)
    ok = np.isfinite(a) & (np.abs(a) < 20) & np.isfinite(b) & (np.abs(b) < 20)
    assert np.allclose(y[ok, 0, 0].view(np.float32), np.sin(a[ok].astype(np.float64)), atol=2e-6)
    assert np.allclose(y[ok, 0, 3].view(np.float32), np.cos(b[ok].astype(np.float64)), atol=2e-6)
