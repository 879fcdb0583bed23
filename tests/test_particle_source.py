"""The particle source on the host (csrc/particle_draw.hpp through gfhip_source_fill_host) against the numpy model of
tests/source_model.py byte for byte, fp64 and fp32 columns: the generator's known answers, counts around a wave, particle
indices whose low word wraps, few and many attempts, a profile, both label kinds; shards; what placed and unplaced
particles hold; uniformity in volume, pitch and speed; the refusals; the plain C++ rule under the sanitizers
(tests/particle_source_check.cpp, a program of its own).  No GPU."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import flux_model
import phase_model
import source_model

DTYPES = {"f64": np.float64, "f32": np.float32}
KNOWN = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,)*4, (0xffffffff,)*2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
COUNTS = (1, 63, 64, 65, 257, 1000)
FIRSTS = (0, 1, 2**32 - 3, 2**40)                                           # the low word of p wraps inside a fill of the third
ATTEMPTS = (1, 2, 64)
SPEED = (0.3, 0.9)
#  On the fixture, measured on the model with 2e5 particles and 64 attempts: 1.88 position attempts per particle and nobody
#  unplaced in EASY; 34.1 (an unplaced particle counts 64) and 23.4 % unplaced in HARD.
EASY = dict(box=(1.2, 2.3, -1.0, 1.0), label_range=(0.0, 0.4))
HARD_RANGE = (0.0, 0.06)
PROFILE = (np.array([0.05, 0.1, 0.18, 0.25, 0.3, 0.35]), np.array([1.0, 0.5, 0.25, 0.0, 0.75]))    # labels off its edges: no cell


@pytest.fixture(scope="module")
def built():
    from graph_framework_amd import build
    build.build_library()


@pytest.fixture(scope="module")
def tables():
    return dict(np.load(os.path.join(GOLDEN, "efit_tables.npz")))


def whole_map(tables):
    numr, numz = tables["psi_c00"].shape
    rmin, dr, zmin, dz = (float(tables[k]) for k in ("rmin", "dr", "zmin", "dz"))
    return rmin, rmin + numr*dr, zmin, zmin + numz*dz


def hard(tables):
    return dict(box=whole_map(tables), label_range=HARD_RANGE)


def cases(tables):
    """24 argument sets that take turns over the counts, the first particles, the attempts, a profile, the label kind, the
    placed column and the two regions: every count meets every number of attempts."""
    out = []
    for i in range(24):
        region = hard(tables) if i % 8 == 5 else EASY
        out.append(dict(region, speed_range=SPEED, count=COUNTS[i % 6], first_particle=FIRSTS[i % 4], attempts=ATTEMPTS[(i//6) % 3],
                        profile=PROFILE if (i//3) % 2 else None, sqrt_label=bool((i//2) % 2), seed=0x9E3779B97F4A7C15 + i,
                        pitch_range=(-1.0, 1.0) if i % 3 else (-0.25, 0.5)))
    return out


def same_fill(got, want):
    """(columns, placed, counters) of two fills, byte for byte."""
    for name, a, b in zip(("x", "y", "z", "ux", "uy", "uz", "gamma"), got[0], want[0]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    assert (got[1] is None) == (want[1] is None) and (got[1] is None or got[1].tobytes() == want[1].tobytes())
    assert got[2] == want[2]


def test_known_answers_through_the_library_and_the_model(built):
    from graph_framework_amd.source import block_host
    for counter, key, answer in KNOWN:
        assert " ".join("%08x" % int(w) for w in block_host(counter, key)) == answer
        assert " ".join("%08x" % int(w) for w in source_model.philox(counter, key)) == answer


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_host_equals_the_model(built, tables, kind):
    from graph_framework_amd.source import fill_host
    seen = dict(placed=0, unplaced=0)
    for number, case in enumerate(cases(tables)):
        with_placed = number % 5 != 0
        got = fill_host(tables, dtype=DTYPES[kind], placed=with_placed, **case)
        columns, placed, counters = source_model.fill(tables, dtype=DTYPES[kind], **case)
        same_fill(got, (columns, placed if with_placed else None, counters))
        assert counters["placed"] + counters["unplaced"] == case["count"]
        seen["placed"] += counters["placed"]
        seen["unplaced"] += counters["unplaced"]
    assert seen["placed"] > 1500 and seen["unplaced"] > 1500


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_two_shards_are_one_fill(built, tables, kind):
    from graph_framework_amd.source import fill_host
    arguments = dict(hard(tables), speed_range=SPEED, seed=77, attempts=16, dtype=DTYPES[kind], profile=PROFILE)
    n, first = 1000, 2**32 - 300
    whole = fill_host(tables, count=n, first_particle=first, **arguments)
    for k in (1, 64, 299, 300, 301, 999):
        low = fill_host(tables, count=k, first_particle=first, **arguments)
        high = fill_host(tables, count=n - k, first_particle=first + k, **arguments)
        joined = ([np.concatenate(pair) for pair in zip(low[0], high[0])], np.concatenate([low[1], high[1]]),
                  {name: low[2][name] + high[2][name] for name in low[2]})
        same_fill(joined, whole)


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_placed_particles_pass_the_test_on_their_stored_columns_and_unplaced_ones_are_nan(built, tables, kind):
    from graph_framework_amd.source import fill_host
    for sqrt_label in (False, True):
        columns, placed, counters = fill_host(tables, **hard(tables), speed_range=SPEED, count=4000, seed=5, attempts=64,
                                              dtype=DTYPES[kind], sqrt_label=sqrt_label)
        assert set(np.unique(placed)) == {0.0, 1.0} and counters["placed"] == int(placed.sum()) > 300
        assert counters["unplaced"] == 4000 - counters["placed"] > 300
        kept = placed == 1
        label = flux_model.label(tables, *[c[kept] for c in columns[:3]], sqrt_label=sqrt_label)
        assert ((HARD_RANGE[0] <= label) & (label < HARD_RANGE[1])).all()
        assert all(np.isfinite(c[kept]).all() for c in columns) and (columns[6][kept] == 0).all()
        nan = np.full(int((~kept).sum()), np.nan, dtype=DTYPES[kind]).tobytes()
        assert all(c[~kept].tobytes() == nan for c in columns)


def volume_fractions(tables, edges, sub, window):
    from graph_framework_amd.flux import volumes_host
    limbs, _ = volumes_host(tables, edges, sub, window=window)
    volume = np.array([float(Fraction(sum(int(limb) << (32*k) for k, limb in enumerate(cell)), 2**1074)) for cell in limbs])
    return volume/volume.sum()


def test_placed_particles_are_uniform_in_volume(built, tables):
    """2e5 particles of the model in EASY over 8 cells of the label against the quadrature of the flux volumes in the same
    box: every count within 5 binomial standard deviations.  sub = 64: doubling it moves no fraction by more than a tenth
    of a standard deviation (measured: at most 0.06 from 64 to 128, 0.1 from 32 to 64; the largest deviation of a count is
    1.8)."""
    n, sub = 200000, 64
    edges = np.linspace(*EASY["label_range"], 9)
    columns, placed, counters = source_model.fill(tables, **EASY, speed_range=SPEED, count=n, seed=2026)
    assert counters["unplaced"] == 0
    counts = np.bincount(flux_model.cells_of(edges, flux_model.label(tables, *columns[:3])), minlength=8)
    fraction, finer = (volume_fractions(tables, edges, s, EASY["box"]) for s in (sub, 2*sub))
    sigma = np.sqrt(n*fraction*(1.0 - fraction))
    print("moved by doubling sub, in sigma:", n*np.abs(finer - fraction)/sigma, "deviations, in sigma:", (counts - n*fraction)/sigma)
    assert counts.sum() == n and (n*np.abs(finer - fraction) <= 0.1*sigma).all()
    assert (np.abs(counts - n*fraction) <= 5.0*sigma).all()


#  The largest |xi - drawn xi| and ||u| - drawn beta| of 2e5 placed particles of the model in EASY, phase_model.label_pitch on
#  the stored columns: rounding alone for fp64; for fp32 the rounding of the six columns to 2^-24 relative.
MODEL_DEVIATION = {"f64": (5.6e-16, 5.6e-16), "f32": (7.8e-8, 4.2e-8)}


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_pitch_and_speed_of_the_stored_columns_are_the_drawn_ones(built, tables, kind):
    from graph_framework_amd.source import fill_host
    n = 200000
    arguments = dict(EASY, speed_range=SPEED, count=n, seed=2026, dtype=DTYPES[kind])
    _, _, _, drawn = source_model.fill(tables, details=True, **arguments)
    columns, placed, counters = fill_host(tables, **arguments)
    assert counters["unplaced"] == 0
    _, xi = phase_model.label_pitch(tables, *columns[:6])
    u = [c.astype(np.float64) for c in columns[3:6]]
    size = np.sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2])
    off_pitch, off_speed = np.abs(xi - drawn["xi"]).max(), np.abs(size - drawn["beta"]).max()
    print(kind, "largest deviation of the pitch %.3e, of the speed %.3e" % (off_pitch, off_speed))
    assert off_pitch <= 2.0*MODEL_DEVIATION[kind][0] and off_speed <= 2.0*MODEL_DEVIATION[kind][1]
    assert SPEED[0] <= drawn["beta"].min() and drawn["beta"].max() < SPEED[1] and abs(drawn["xi"].mean()) < 0.01
    assert abs(drawn["beta"].mean() - 0.6) < 0.002


def test_regions_are_what_the_cases_take_them_for(tables):
    """Nobody is unplaced in EASY after 64 attempts, about a quarter in HARD: the model alone."""
    n = 20000
    _, _, easy = source_model.fill(tables, **EASY, speed_range=SPEED, count=n, seed=1)
    _, _, tough = source_model.fill(tables, **hard(tables), speed_range=SPEED, count=n, seed=1)
    assert easy["unplaced"] == 0 and 1.8 < easy["position_tries"]/n < 2.0
    assert 0.2 < tough["unplaced"]/n < 0.27 and 30 < tough["position_tries"]/n < 38


def test_refusals(built, tables):
    from graph_framework_amd import GfHipError
    from graph_framework_amd.source import PLAIN, REFILL, fill_host

    def refused(match, error=GfHipError, **changed):
        arguments = dict(EASY, tables=tables, speed_range=SPEED, count=5)
        arguments.update(changed)
        with pytest.raises(error, match=match):
            fill_host(**arguments)

    nan = float("nan")
    for box in ((1.2, 1.2, -1, 1), (2.3, 1.2, -1, 1), (1.2, 2.3, 1, 1), (nan, 2.3, -1, 1), (1.2, 2.3, -1, float("inf")), (-0.1, 2.3, -1, 1)):
        refused("box", box=box)
    for label_range in ((0.4, 0.4), (0.4, 0.0), (nan, 0.4), (0.0, nan)):
        refused("label range", label_range=label_range)
    for speed_range in ((0.5, 0.5), (0.9, 0.3), (nan, 0.9), (0.3, nan), (-0.1, 0.9), (0.3, 1.0)):
        refused("speed range", speed_range=speed_range)
    for pitch_range in ((0.5, 0.5), (0.5, -0.5), (nan, 0.5), (-0.5, nan), (-1.5, 0.5), (-0.5, 1.5)):
        refused("pitch range", pitch_range=pitch_range)
    refused("1 to 4096 attempts", attempts=0)
    refused("1 to 4096 attempts", attempts=4097)
    for value in (-0.1, 1.1, nan):
        refused(r"\[0, 1\]", profile=(PROFILE[0], np.array([1.0, value, 0.25, 0.0, 0.75])))
    refused("at most 256 cells", profile=(np.linspace(0.0, 0.4, 258), np.full(257, 0.5)))
    refused("strictly increasing", profile=(PROFILE[0][::-1], PROFILE[1]))
    refused("one edge more", ValueError, profile=(PROFILE[0], PROFILE[1][:-1]))
    refused("unknown flag", flags=4)
    refused("one route", flags=PLAIN | REFILL)
    refused("overflows 64 bits", first_particle=2**64 - 3)
    refused("finite and non-zero", span=0.0)                                # the map, as a distribution's
    refused("dpsi", tables=dict(tables, dpsi=np.float64(0.0)), span=1.0)    # the field
    refused("fp32 or fp64", ValueError, dtype=np.int32)
    columns, placed, counters = fill_host(tables, **EASY, speed_range=SPEED, count=5, attempts=4096, profile=(np.array([0.0, 0.4]), np.array([1.0])))
    assert counters["placed"] == 5


def test_the_plain_cpp_rule_under_the_sanitizers(tmp_path):
    """tests/particle_source_check.cpp: source_host.hpp on an analytic map, fp32 and fp64, with and without a profile,
    against a plain restatement of what a fill promises, built with -fsanitize=address,undefined and run as a child."""
    binary = str(tmp_path/"particle_source_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "graph_framework_amd", "csrc"), "-o", binary,
                           os.path.join(ROOT, "tests", "particle_source_check.cpp")])
    out = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-3000:])
    assert out.returncode == 0
    last = out.stdout.split()
    assert last[-4] == "cases" and int(last[-3]) > 1000 and last[-2:] == ["failures", "0"]
