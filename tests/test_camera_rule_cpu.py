"""The shared camera and volume arithmetic without a GPU: tests/camera_rule_harness.cpp compiles the functions of
stereo-depth_amd/csrc/k_camera.h (the code the 3D kernels run) for the host with the library's flags and evaluates them
on the cases below; this file restates every function in NumPy, one np.float32 operation per step, and demands equal
bits (any NaN equals any NaN).

The contraction cases are operands on which fusing a multiply into the add that follows changes the result.  The fused
value is computed here (the exact product in float64, one rounding to float32 after the add) and must differ from the
expected one, so a case that would not notice a contracted build fails instead of passing silently.

Built like the other rule harnesses (host code only, no HIP runtime linked), with the address and undefined-behaviour
sanitizers when their runtimes link that way and without them otherwise.  Where the host CPU has fused multiply-add
instructions the harness is built with -mfma: a plain x86-64 target has none, so without it a build that lost
-ffp-contract=off could not contract anything and the contraction cases would prove nothing.  No GPU."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "camera_rule_harness.cpp")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
f32 = np.float32
HALF, ZERO, TOP = f32(0.5), f32(0.0), f32(255.0)


def _build_module():
    spec = importlib.util.spec_from_file_location("smx_build", os.path.join(ROOT, "stereo-depth_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def host_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma " in line + " " for line in f)
    except OSError:
        return False


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not found")
    b = _build_module()
    exe = str(tmp_path_factory.mktemp("camera_rule") / "camera_rule")
    log = ""
    fma = ["-mfma"] if host_has_fma() else []
    for extra in (SANITIZE, []):
        cmd = [b.hipcc(), "-x", "hip", "--cuda-host-only", "-no-hip-rt"] + b.FLAGS + fma + extra + ["-I", b.INCLUDE, "-I", b.CSRC,
                                                                                                      "-o", exe, HARNESS]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode == 0:
            print("camera-rule harness built", "with -fsanitize=address,undefined" if extra else "WITHOUT the sanitizers",
                  "and with -mfma" if fma else "and WITHOUT -mfma")
            return exe
        log += " ".join(cmd) + "\n" + r.stdout + r.stderr + "\n"
    raise AssertionError("harness did not compile:\n" + log[-6000:])


# ---- the restatement: every line is one float32 operation --------------------------------------------------------------
def affine(m, x, y, z):
    a = m[0] * x
    b = m[1] * y
    s = a + b
    c = m[2] * z
    s = s + c
    return s + m[3]


def ray(m, u, v):                    # m = (m0, m1, m3)
    a = m[0] * u
    b = m[1] * v
    s = a + b
    return s + m[2]


def rot(m, a, b):                    # m = (m0, m1, m2)
    p = m[0] * a
    q = m[1] * b
    s = p + q
    return s + m[2]


def near(p, p3):
    q = p / p3
    q = q + HALF
    return np.floor(q)


def fmaxf(a, b):                     # C's: the other operand when one is a NaN
    return b if np.isnan(a) else a if np.isnan(b) else max(a, b)


def fminf(a, b):
    return b if np.isnan(a) else a if np.isnan(b) else min(a, b)


def byte(v):
    t = v + HALF
    t = np.floor(t)
    t = fmaxf(t, ZERO)
    t = fminf(t, TOP)
    return int(t)


def plane(m, ch, channels):
    return m * 3 + ch if channels == 3 else m


def centre(o, i, s):
    t = f32(i) + HALF
    t = t * s
    return o + t


def index(k, j, i, ny, nx):
    return (k * ny + j) * nx + i     # Python integers: exact


def search(tab, lo, hi, p):
    return max(m for m in range(lo, hi + 1) if tab[m] <= p)


def fused(a, b, c):
    """fma(a, b, c) as the issue defines it: the exact product in float64, rounded to float32 once, after the add."""
    return f32(np.float64(a) * np.float64(b) + np.float64(c))


# every way to fuse ONE multiply of a function into the add that follows it
def affine_fused(m, x, y, z):
    inner = m[0] * x + m[1] * y
    return [(fused(m[0], x, m[1] * y) + m[2] * z) + m[3], (fused(m[1], y, m[0] * x) + m[2] * z) + m[3],
            fused(m[2], z, inner) + m[3]]


def ray_fused(m, u, v):
    return [fused(m[0], u, m[1] * v) + m[2], fused(m[1], v, m[0] * u) + m[2]]


def rot_fused(m, a, b):
    return ray_fused(m, a, b)


# ---- the cases ----------------------------------------------------------------------------------------------------------
def bits(x):
    return int(np.asarray(x, f32).view(np.uint32))


def hexf(*xs):
    return " ".join(f"{bits(x):08x}" for x in xs)


def from_bits(b):
    return np.array([b], np.uint32).view(f32)[0]


SPECIAL = [from_bits(b) for b in (0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc00000)]


def operand_sets(rng, count):
    """count float32 operands each, over several magnitudes, then every special value in every operand position."""
    sets = []
    for scale in (1e-30, 1e-3, 1.0, 640.0, 1e6, 1e30):
        for _ in range(6):
            sets.append((rng.standard_normal(count) * scale).astype(f32))
    for pos in range(count):
        for s in SPECIAL:
            v = rng.standard_normal(count).astype(f32)
            v[pos] = s
            sets.append(v)
    return sets


def sensitive(rng, fn, fn_fused, n_m, n_v, want):
    """`want` operand sets near 1 on which every single fusion changes the result (a fixed seed: the same sets every run)."""
    out = []
    while len(out) < want:
        v = (f32(1.0) + rng.integers(-4096, 4096, n_m + n_v).astype(f32) * f32(2.0 ** -12)) * rng.choice([-1.0, 1.0], n_m + n_v).astype(f32)
        v = v.astype(f32)
        want_bits = bits(fn(v[:n_m], *v[n_m:]))
        if all(bits(t) != want_bits for t in fn_fused(v[:n_m], *v[n_m:])):
            out.append(v)
    return out


def build_cases():
    """[(input line, expected output line, note)]"""
    rng = np.random.default_rng(20240917)
    cases = []
    with np.errstate(all="ignore"):
        for k, v in enumerate(operand_sets(rng, 7)):
            cases.append((f"affine {k % 4} " + hexf(*v), f"{bits(affine(v[:4], *v[4:])):08x}", "affine"))
        for k, v in enumerate(operand_sets(rng, 5)):
            cases.append((f"ray {k % 4} " + hexf(*v), f"{bits(ray(v[:3], *v[3:])):08x}", "ray"))
            cases.append((f"rot {k % 4} " + hexf(*v), f"{bits(rot(v[:3], *v[3:])):08x}", "rot"))
        # rounding: random quotients, exact .5 ties on both sides of zero, a denormal p3, the specials
        near_cases = [tuple(v) for v in operand_sets(rng, 2)]
        near_cases += [(f32(t), f32(1.0)) for t in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 8388607.5, 0.49999997, -0.49999997)]
        near_cases += [(f32(t * 3.0), f32(3.0)) for t in (0.5, 1.5, 2.5, -0.5, 639.5)]
        near_cases += [(f32(p), from_bits(b)) for p in (1.0, -1.0, 1e-38, 0.0) for b in (0x00000001, 0x007fffff, 0x80000001)]
        for p, p3 in near_cases:
            cases.append(("near " + hexf(p, p3), f"{bits(near(p, p3)):08x}", "near"))
        byte_cases = [-0.5, -0.4999, 254.5, 255.5, 1e30, np.nan, -0.50001, 0.5, 0.49999997, 1.5, 254.49998, 127.5, 255.0, 256.0,
                      -1e30, np.inf, -np.inf, -0.0, 1e-45] + list(rng.uniform(-20.0, 280.0, 40))
        for v in byte_cases:
            b = byte(f32(v))
            assert 0 <= b <= 255
            cases.append(("byte " + hexf(v), f"{b:x} {b:x}", "byte"))
        for m, ch, channels in [(0, 0, 1), (5, 0, 1), (5, 2, 1), (0, 0, 3), (5, 0, 3), (5, 1, 3), (5, 2, 3), (7, 1, 0), (2 ** 30, 2, 3)]:
            cases.append((f"plane {m} {ch} {channels}", f"{plane(m, ch, channels):x}", "plane"))
        for v in operand_sets(rng, 2):
            i = int(rng.integers(0, 4096))
            cases.append((f"centre {hexf(v[0])} {i} {hexf(v[1])}", f"{bits(centre(v[0], i, v[1])):08x}", "centre"))
        for i in (0, 1, 511, 4095, 16777217, 2 ** 31 - 1):             # (float)i rounds above 2^24
            cases.append((f"centre {hexf(-3.2)} {i} {hexf(0.0125)}", f"{bits(centre(f32(-3.2), i, f32(0.0125))):08x}", "centre"))
        # voxel indices: the far corner of (4096, 4096, 64) is 2^30 - 1; of (4096, 4096, 256) and (2048, 2048, 2048) it
        # lies above 2^31 and above 2^32, where an index computed in 32 bits wraps
        for nx, ny, nz in [(4096, 4096, 64), (4096, 4096, 256), (2048, 2048, 2048), (7, 5, 3), (1, 1, 1)]:
            for k, j, i in [(nz - 1, ny - 1, nx - 1), (nz - 1, 0, 0), (0, ny - 1, nx - 1), (nz // 2, ny // 3, nx // 5)]:
                cases.append((f"index {k} {j} {i} {ny} {nx}", f"{index(k, j, i, ny, nx):x}", "index"))
        # the search: repeated entries, lo == hi, p equal to the first and to the last entry, sub-ranges
        tables = [[0], [0, 0, 0, 0], [0, 3, 3, 3, 7, 7, 12], [-5, -5, 0, 1, 1, 1, 1, 9, 200, 200], list(range(0, 64, 3)),
                  [0, 100, 100, 100, 100, 100, 100, 2 ** 31 - 1]]
        for tab in tables:
            n = len(tab)
            spans = {(0, n - 1), (0, 0), (n - 1, n - 1), (n // 2, n // 2), (n // 3, n - 1), (0, n // 2), (n // 3, (2 * n) // 3)}
            for lo, hi in sorted(spans):
                for p in sorted({tab[lo], tab[hi], tab[lo] + 1, tab[hi] - 1, tab[(lo + hi) // 2], tab[hi] + 5}):
                    if p < tab[lo] or p > 2 ** 31 - 1:
                        continue                                       # the precondition: tab[lo] <= p
                    cases.append((f"search {lo} {hi} {p} {n} " + " ".join(map(str, tab)), f"{search(tab, lo, hi, p):x}", "search"))
    return cases


def contraction_cases():
    """[(input line, expected output line, [the fused variants that must differ from it])] per multiply-add function"""
    rng = np.random.default_rng(77)
    e12, e11 = f32(1.0 + 2.0 ** -12), f32(1.0 + 2.0 ** -11)
    out = {"affine": [], "ray": [], "rot": []}
    # the issue's construction: the product 1 + 2^-11 + 2^-24 rounds to even, so unfused 0 and fused 2^-24
    v = np.array([e12, -e11, 0.0, 0.0, e12, 1.0, 0.0], f32)
    assert bits(affine(v[:4], *v[4:])) == 0 and bits(affine_fused(v[:4], *v[4:])[0]) == bits(f32(2.0 ** -24))
    out["affine"].append((v, affine_fused(v[:4], *v[4:])[:1]))
    v = np.array([e12, -e11, 0.0, e12, 1.0], f32)
    out["ray"].append((v, ray_fused(v[:3], *v[3:])[:1]))
    out["rot"].append((v, rot_fused(v[:3], *v[3:])[:1]))
    # operand sets on which EVERY single fusion changes the bits
    for v in sensitive(rng, affine, affine_fused, 4, 3, 10):
        out["affine"].append((v, affine_fused(v[:4], *v[4:])))
    for v in sensitive(rng, ray, ray_fused, 3, 2, 10):
        out["ray"].append((v, ray_fused(v[:3], *v[3:])))
    for v in sensitive(rng, rot, rot_fused, 3, 2, 10):
        out["rot"].append((v, rot_fused(v[:3], *v[3:])))
    fn = {"affine": (affine, 4), "ray": (ray, 3), "rot": (rot, 3)}
    lines = []
    for name, sets in out.items():
        f, n_m = fn[name]
        for k, (v, variants) in enumerate(sets):
            lines.append((f"{name} {k % 4} " + hexf(*v), f"{bits(f(v[:n_m], *v[n_m:])):08x}", name, [bits(t) for t in variants]))
    return lines


def run(harness, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(lines), (len(got), len(lines))
    return got


def same(got, want, note):
    if note in ("affine", "ray", "rot", "near", "centre"):                  # NaN as NaN, whatever its payload and sign
        g, w = from_bits(int(got, 16)), from_bits(int(want, 16))
        if np.isnan(g) and np.isnan(w):
            return True
    return got == want


def test_every_function_matches_its_restatement(harness):
    cases = build_cases()
    kinds = {note: sum(1 for c in cases if c[2] == note) for note in {c[2] for c in cases}}
    print(len(cases), "cases:", kinds)
    assert 300 <= len(cases) <= 2000 and set(kinds) == {"affine", "ray", "rot", "near", "byte", "plane", "centre", "index", "search"}
    got = run(harness, [c[0] for c in cases])
    bad = [(c[0], g, c[1]) for c, g in zip(cases, got) if not same(g, c[1], c[2])]
    assert not bad, f"{len(bad)} of {len(cases)} cases differ (case, got, expected): {bad[:5]}"


def test_the_far_corner_indices_pass_31_bits():
    assert index(63, 4095, 4095, 4096, 4096) == 2 ** 30 - 1
    assert index(255, 4095, 4095, 4096, 4096) == 2 ** 32 - 1 and index(2047, 2047, 2047, 2048, 2048) == 2 ** 33 - 1


def test_a_contracted_build_would_be_noticed(harness):
    cases = contraction_cases()
    for name in ("affine", "ray", "rot"):
        mine = [c for c in cases if c[2] == name]
        assert len(mine) >= 8, name
        for line, want, _, variants in mine:                               # a case that is not sensitive fails here
            assert variants and all(v != int(want, 16) for v in variants), (line, want, variants)
        # at least eight of them notice EVERY single fusion (affine: three places, the others: two)
        assert sum(1 for c in mine if len(c[3]) == (3 if name == "affine" else 2)) >= 8, name
    got = run(harness, [c[0] for c in cases])
    bad = [(c[0], g, c[1]) for c, g in zip(cases, got) if g != c[1]]
    assert not bad, f"{len(bad)} contraction cases differ (case, got, expected): {bad[:5]}"
