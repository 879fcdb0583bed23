"""Batches of rays on the host alone.  csrc/ray_batches.hpp — the batch of a ray, the rays of a batch in closed form and
the walk of the batched deposit kernels — driven by tests/ray_batches_check.cpp, built with
-fsanitize=address,undefined and run as a child process; graph_framework_amd/batches.py held to the model of
tests/flux_batch_model.py: the rays of a batch to a count ray by ray, the standard error to rational arithmetic, and to
the true spread of a seeded tally; and the writers' new variables.  No GPU."""
import decimal
import os
import subprocess
import sys

import numpy as np
import pytest

import flux_batch_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRSTS = (0, 1, 63, 64, 65, 2**40 + 5)
BATCHES = (1, 2, 3, 16, 64, 256)


def counts_for(batches):
    return (1, 63, 64, 65, 64*batches - 1, 64*batches, 64*batches + 1, 4099)


def test_the_walk_and_batch_rays_under_the_sanitizers(tmp_path):
    """first_ray in {0, 1, 63, 64, 65, 2^40 + 5} x count in {1, 63, 64, 65, 64G - 1, 64G, 64G + 1, 4099} x G in {1, 2, 3,
    16, 64, 256} x {1, 2, 300} workgroups x {1, 4, 16} waves: every sample once, by a unit of its own batch, the
    close() calls (the barriers) the same for every wave of a workgroup, batch_rays the count ray by ray."""
    binary = str(tmp_path/"ray_batches_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", binary, os.path.join(ROOT, "tests", "ray_batches_check.cpp")])
    out = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:], out.stderr[-3000:])
    assert out.returncode == 0
    last = out.stdout.split()
    assert last[-8:-6] == ["cases", str(6*6*8*3*3)] and last[-2:] == ["failures", "0"]


def test_batch_rays_is_the_count_ray_by_ray():
    from graph_framework_amd.batches import batch_of, batch_rays
    for first in FIRSTS:
        for batches in BATCHES:
            for count in counts_for(batches) + (0,):
                got = batch_rays(first, count, batches)
                assert got.dtype == np.int64 and got.shape == (batches,)
                assert (got == model.batch_rays(first, count, batches)).all(), (first, count, batches)
    rays = np.arange(2**40, 2**40 + 1000, dtype=np.uint64)
    assert (batch_of(rays, 3).astype(np.int64) == model.batch_index(2**40, 1000, 3)).all()
    assert batch_of(64*5 + 63, 3) == 2 and batch_of(64*6, 3) == 0


def planted_cases():
    """{name: (sums (G, cells), total (cells,), rays (G,), count)}: S_g and S are planted numbers, not sums of one
    another — the formula takes them as they are."""
    rng = np.random.default_rng(7)
    cases = {}
    for name, rays in (("equal", [640]*16), ("unequal", [64, 640, 6400, 63, 1, 4099, 100, 7]), ("one_empty", [128, 0, 64, 17, 128])):
        rays = np.array(rays)
        count = int(rays.sum())
#  (the bound counts roundings: the squares of the deviations stay clear of under- and overflow)
        means = rng.uniform(0.5, 1.5, (rays.size, 6))*np.array([1.0, 1e-9, 1e12, -3.0, 1e-100, 2.0**200])
        sums = means*rays[:, None]
        sums[:, 3] += rng.uniform(-40.0, 40.0, rays.size)                   # large spread, both signs
        sums[rays == 0] = 0.0
        total = sums.sum(axis=0)*(1.0 + rng.uniform(-1e-3, 1e-3, 6))          # S is given, not the sum of the rounded parts
        cases[name] = (sums, total, rays, count)
#  all p_g equal, every quotient exact: stderr is 0.0 to the bit; next to it a cell where they differ
    rays = np.array([64, 128, 192, 17])
    sums = np.stack([3.0*rays, 3.0*rays + np.array([1.0, -1.0, 0.5, 0.0])], axis=1)
    cases["all_equal"] = (sums, np.array([3.0*rays.sum(), 3.0*rays.sum() + 0.5]), rays, int(rays.sum()))
    return cases


@pytest.mark.parametrize("name", ["equal", "unequal", "one_empty", "all_equal"])
def test_standard_error_against_rational_arithmetic(name):
    """batches.standard_error_of in fp64 against the same formula in fractions.Fraction, the square root taken last at 50
    digits.  The bound is flux_batch_model.error_bound's, derived there from the roundings of the numpy expression:
    gamma*exact + (1 + gamma)*sqrt(sum n_g delta_g^2/((m - 1) N)), gamma = 1.0001 (m + 5)/2 u, delta_g = 1.0001 u (|p_g| +
    |P| + |p_g - P|), u = 2^-53, m the batches with rays."""
    from graph_framework_amd.batches import standard_error_of
    sums, total, rays, count = planted_cases()[name]
    mean, stderr, used = standard_error_of(sums, total, rays, count)
    assert used == int((rays > 0).sum()) and stderr.shape == total.shape and mean.shape == total.shape
    worst = 0.0
    for cell in range(total.size):
        exact_mean, exact, exact_used = model.exact_standard_error(sums[:, cell], total[cell], rays, count)
        assert exact_used == used
        assert mean[cell] == float(exact_mean)                                  # one correctly rounded division
        bound = model.error_bound(sums[:, cell], total[cell], rays, count)
        error = abs(decimal.Decimal(float(stderr[cell])) - exact)
        ulps = float(error)/np.spacing(float(exact)) if exact else 0.0
        print(name, "cell", cell, "stderr", stderr[cell], "error", float(error), "=", ulps, "ulp; bound", float(bound))
        assert error <= bound, (name, cell)
        worst = max(worst, ulps)
    print(name, "largest error", worst, "ulp of the exact stderr")
    if name == "all_equal":
        assert stderr[0] == 0.0 and not np.signbit(stderr[0]) and stderr[1] > 0.0


def test_standard_error_of_fewer_than_two_batches_is_nan():
    from graph_framework_amd.batches import standard_error_of
    sums = np.array([[0.0, 0.0], [7.5, -2.0], [0.0, 0.0]])
    mean, stderr, used = standard_error_of(sums, sums[1], [0, 60, 0], 60)
    assert used == 1 and np.isnan(stderr).all() and stderr.shape == (2,)
    assert (mean == sums[1]/60.0).all()
    mean, stderr, used = standard_error_of(sums[1:2], sums[1], [60], 60)         # G = 1
    assert used == 1 and np.isnan(stderr).all()
    assert model.exact_standard_error(sums[:, 0], 7.5, [0, 60, 0], 60)[1] is None
    spectrum = np.arange(24.0).reshape(2, 3, 4)                                  # a batch axis before two cell axes
    mean, stderr, used = standard_error_of(spectrum, spectrum.sum(axis=0), [64, 64], 128)
    assert used == 2 and stderr.shape == (3, 4) and np.isfinite(stderr).all()
    with pytest.raises(ValueError):
        standard_error_of(spectrum, spectrum[0], [64, 64, 64], 192)


@pytest.mark.parametrize("seed", range(20))
def test_the_batch_stderr_is_the_true_spread(seed):
    """65536 rays, 64 batches, 8 cells; every ray puts one uniform value into one uniformly chosen cell.  The batch
    stderr over std(contribution)/sqrt(N), the contribution of a ray to a cell being its value or 0, lies in [2/3, 3/2]
    in every cell."""
    from graph_framework_amd.batches import batch_rays, standard_error_of
    rays, batches, cells = 65536, 64, 8
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, cells, rays)
    value = rng.uniform(0.0, 1.0, rays)
    sums, total = model.tally(cell, value, cells, 0, batches)
    mean, stderr, used = standard_error_of(sums, total, batch_rays(0, rays, batches), rays)
    assert used == batches
    contribution = np.where(cell[None, :] == np.arange(cells)[:, None], value[None, :], 0.0)
    true = contribution.std(axis=1)/np.sqrt(rays)
    assert np.allclose(mean, contribution.mean(axis=1), rtol=1e-12)
    ratio = stderr/true
    print("seed", seed, "ratio", ratio.min(), ratio.max())
    assert (ratio >= 2.0/3.0).all() and (ratio <= 1.5).all()


def test_largest_relative_error():
    from graph_framework_amd.batches import largest_relative_error
    mean = np.array([10.0, -5.0, 0.05, 0.0])
    stderr = np.array([0.1, 0.2, 0.04, np.nan])
    assert largest_relative_error(mean, stderr) == 0.2/5.0                       # 0.05 is below 1 % of the peak
    assert np.isnan(largest_relative_error(np.zeros(3), np.full(3, np.nan)))


def written(path):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    return H5File(path)


def same_file(write, plain, again):
    for _ in range(3):                                                      # a dataset's header holds the second it was created in
        write(plain, {})
        write(again, dict(stderr=None, batch_bins=None, batch_rays=None))
        if int(os.path.getmtime(plain)) == int(os.path.getmtime(again)):
            break
    assert open(plain, "rb").read() == open(again, "rb").read()


def test_flux_bins_file_with_batches(tmp_path):
    """write_flux_bins with stderr, batch_bins and batch_rays: three more f8 variables, on ns, (nb, ns) and nb; without
    them the bytes of the file as it was."""
    from graph_framework_amd.output import write_flux_bins
    bins = np.array([0.5, 5e-324, -3.0, 0.0])
    edges = np.linspace(0.0, 1.0, 5)**2
    stderr = np.array([0.25, 0.0, np.nan, 1e-300])
    batch_bins = np.arange(12.0).reshape(3, 4) - 2.5
    batch_bins[1, 2] = np.nan
    batch_rays = np.array([64, 0, 17])
    counts = dict(samples=9, outside=1, skipped=0)
    plain, again, full = (str(tmp_path/name) for name in ("plain.nc", "again.nc", "full.nc"))
    same_file(lambda path, options: write_flux_bins(path, bins, edges, 0.125, 0.5, "s", **counts, **options), plain, again)
    write_flux_bins(full, bins, edges, 0.125, 0.5, "s", stderr=stderr, batch_bins=batch_bins, batch_rays=batch_rays,
                    volume=bins, density=bins, sub=3, **counts)
    f = written(full)
    for name, want in (("bins", bins), ("sbins", edges), ("volume", bins), ("stderr", stderr), ("batch_bins", batch_bins),
                       ("batch_rays", batch_rays.astype(np.float64))):
        got = f.read(name)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
    f.close()
    write_flux_bins(full, bins, edges, 0.125, 0.5, "s", stderr=stderr, **counts)       # each of them is optional
    f = written(full)
    assert f.read("stderr").tobytes() == stderr.tobytes()
    f.close()
    with pytest.raises(ValueError):
        write_flux_bins(full, bins, edges, 0.125, 0.5, "s", batch_bins=batch_bins, batch_rays=batch_rays[:2])


def test_spectrum_bins_file_with_batches(tmp_path):
    from graph_framework_amd.output import write_spectrum_bins
    bins = np.arange(6.0).reshape(2, 3)
    sbins, nbins = np.array([0.0, 0.5, 1.0]), np.array([-1.0, 0.0, 0.25, 1.0])
    stderr = bins/7.0
    batch_bins = np.arange(24.0).reshape(4, 2, 3)/3.0
    batch_rays = np.array([128, 64, 64, 1])
    counts = dict(samples=9, outside=1, skipped=0)
    plain, again, full = (str(tmp_path/name) for name in ("plain.nc", "again.nc", "full.nc"))
    same_file(lambda path, options: write_spectrum_bins(path, bins, sbins, nbins, 0.125, 0.5, "s", 2.0, **counts, **options),
              plain, again)
    write_spectrum_bins(full, bins, sbins, nbins, 0.125, 0.5, "s", 2.0, stderr=stderr, batch_bins=batch_bins,
                        batch_rays=batch_rays, **counts)
    f = written(full)
    for name, want in (("bins", bins), ("sbins", sbins), ("nbins", nbins), ("stderr", stderr), ("batch_bins", batch_bins),
                       ("batch_rays", batch_rays.astype(np.float64))):
        got = f.read(name)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
    f.close()
