"""CPU tests of the deposition feature: the superaccumulator core (csrc/superacc.hpp, the functions the
deposit, normalise and round kernels run) through gfhip_exact_sum, against rational arithmetic, and the
bins.nc writer.  math.fsum is no oracle here: it raises or differs on intermediate overflow.

The oracle is exact: every double is an integer multiple of 2^-1074, so a sum is one Python integer N in
those units; float(Fraction(N, 2^1074)) is the correctly rounded double (CPython's int/int division rounds
to nearest even), +-inf from 2^1024 - 2^970 on (the midpoint between DBL_MAX and 2^1024, which ties to the
even 2^1024).  The canonical limbs are the base-2^32 two's-complement digits of N."""
import ctypes
import os
import random
import struct
from fractions import Fraction

import numpy as np
import pytest

LIMBS = 67
DBL_MAX = 1.7976931348623157e308
UNIT = 1 << 1074
OVERFLOW = (1 << 1024) - (1 << 970)


@pytest.fixture(scope="module")
def lib():
    from graph_framework_amd import build, _lib
    build.build_library()
    return _lib.load()


def units(value):
    """A finite double as an integer count of 2^-1074."""
    numerator, denominator = float(value).as_integer_ratio()
    return numerator*(UNIT//denominator)


def rounded(total_units):
    """The correctly rounded double of total_units 2^-1074."""
    exact = Fraction(total_units, UNIT)
    if abs(exact) >= OVERFLOW:
        return float("inf") if exact > 0 else float("-inf")
    return float(exact)


def canonical_limbs(total_units):
    low = total_units & ((1 << (32*(LIMBS - 1))) - 1)
    limbs = [(low >> (32*k)) & 0xffffffff for k in range(LIMBS - 1)]
    return limbs + [total_units >> (32*(LIMBS - 1))]


def bits(value):
    return struct.pack("<d", value)


def exact_sum(lib, values):
    array = np.ascontiguousarray(values, dtype=np.float64)
    total = ctypes.c_double()
    limbs = np.full(LIMBS, 12345, dtype=np.int64)
    assert lib.gfhip_exact_sum(array.ctypes.data, array.size, ctypes.byref(total), limbs.ctypes.data) == 0
    return total.value, limbs


def check(lib, values, expected=None):
    total_units = sum(units(v) for v in values)
    want = rounded(total_units)
    if expected is not None:
        assert bits(want) == bits(expected), (values, want, expected)      # the oracle itself
    got, limbs = exact_sum(lib, values)
    assert bits(got) == bits(want), (values, got, want)
    assert [int(l) for l in limbs] == canonical_limbs(total_units), values
    shuffled = list(values)
    random.Random(len(values)).shuffle(shuffled)
    again, limbs_again = exact_sum(lib, shuffled)
    assert bits(again) == bits(got) and limbs_again.tobytes() == limbs.tobytes(), values


TINY = 5e-324
CASES = [
    ([1e308, 1.0, -1e308], 1.0),
    ([2.0**53, 1.0], 2.0**53),                                   # tie to even
    ([2.0**53, 1.0, TINY], 2.0**53 + 2.0),
    ([DBL_MAX, 2.0**969], DBL_MAX),
    ([DBL_MAX, 2.0**970], float("inf")),
    ([-DBL_MAX, -2.0**970], float("-inf")),
    ([DBL_MAX, DBL_MAX, -DBL_MAX], DBL_MAX),
    ([TINY, TINY, TINY], 1.5e-323),
    ([2.0**-1023, 2.0**-1023], 2.0**-1022),                      # subnormals into the smallest normal
    ([2.2250738585072009e-308, TINY], 2.2250738585072014e-308),  # largest subnormal + one unit
    ([-TINY, -2.0**-1030, TINY], -2.0**-1030),
    ([1.5, -1.5], 0.0),
    ([-2.5, 2.5], 0.0),
    ([DBL_MAX, -DBL_MAX], 0.0),
    ([], 0.0),
    ([-1.0], -1.0),
    ([0.0, -0.0], 0.0),
    ([2.0**53 + 2.0, 1.0], 2.0**53 + 4.0),                       # tie to even, upwards
    ([2.0**52, 0.5, 0.25], 2.0**52 + 1.0),                       # guard and sticky
    ([1.0, 2.0**-53], 1.0),
    ([1.0, 2.0**-53, TINY], 1.0 + 2.0**-52),
    ([-1.0, -2.0**-53, -TINY], -1.0 - 2.0**-52),
]


@pytest.mark.parametrize("values,expected", CASES)
def test_exact_sum_named_cases(lib, values, expected):
    check(lib, values, expected)
    if values and expected == 0.0:
        got, _ = exact_sum(lib, values)
        assert bits(got) == bits(0.0)                            # an exact zero is +0.0


def random_set(rng):
    extremes = [DBL_MAX, -DBL_MAX, 2.0**969, 2.0**970, TINY, -TINY, 2.0**53, 1.0, 1e308, -1e308, 2.0**-1022, 0.0]
    values = []
    for _ in range(rng.randint(1, 40)):
        kind = rng.random()
        if kind < 0.4:
            while True:
                v = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
                if v == v and abs(v) != float("inf"):
                    break
        elif kind < 0.8:
            v = rng.uniform(-1.0, 1.0)*2.0**rng.randint(-60, 60)
        else:
            v = rng.choice(extremes)
        values.append(v)
    if rng.random() < 1.0/3.0:
        values += [-v for v in values if rng.random() < 0.9]
        rng.shuffle(values)
    return values


def test_exact_sum_random_sets(lib):
    rng = random.Random(20260117)
    overflowed = zeros = 0
    for _ in range(3000):
        values = random_set(rng)
        check(lib, values)
        total = rounded(sum(units(v) for v in values))
        overflowed += abs(total) == float("inf")
        zeros += total == 0.0
    assert overflowed > 20 and zeros > 20                        # the sets reach both ends


def test_exact_sum_refuses_non_finite_values(lib):
    total = ctypes.c_double()
    for bad in (float("nan"), float("inf")):
        array = np.array([1.0, bad])
        assert lib.gfhip_exact_sum(array.ctypes.data, 2, ctypes.byref(total), None) != 0


def test_exact_sum_of_many_values_is_order_free(lib):
    """1e5 values over 600 binades: numpy's pairwise sum moves with the order, the exact sum does not."""
    rng = np.random.default_rng(7)
    values = rng.uniform(-1.0, 1.0, 100000)*2.0**rng.integers(-300, 300, 100000)
    got, limbs = exact_sum(lib, values)
    again, limbs_again = exact_sum(lib, values[rng.permutation(values.size)])
    assert bits(got) == bits(again) and limbs.tobytes() == limbs_again.tobytes()
    assert bits(got) == bits(rounded(sum(units(v) for v in values)))


def _hdf5_reader():
    from graph_framework_amd.output import _hdf5
    lib = _hdf5()
    hid = ctypes.c_int64
    lib.H5Aopen.restype = hid
    lib.H5Aopen.argtypes = [hid, ctypes.c_char_p, hid]
    lib.H5Aread.argtypes = [hid, hid, ctypes.c_void_p]
    lib.H5Aexists.argtypes = [hid, ctypes.c_char_p]
    lib.H5Dget_type.restype = hid
    lib.H5Dget_type.argtypes = [hid]
    lib.H5Tget_class.argtypes = [hid]
    lib.H5Tget_size.restype = ctypes.c_size_t
    lib.H5Tget_size.argtypes = [hid]
    lib.hl.H5DSis_attached.argtypes = [hid, hid, ctypes.c_uint]
    lib.hl.H5DSis_scale.argtypes = [hid]
    lib.hl.H5DSget_num_scales.argtypes = [hid, ctypes.c_uint]
    return lib


def test_bins_file_has_the_layout_of_bin_py(tmp_path):
    """output.write_bins writes bins.nc as utilities/bin.py does through netCDF4 (bin.py:19-30, :49-51, :108): the
    dimensions nx, ny, nz, nxp, nyp, nzp, the f8 variables bins(nx, ny, nz), xbins(nxp), ybins(nyp), zbins(nzp) —
    in NetCDF-4's on-disk conventions (dimension scales without coordinate variables, attached to the variables'
    axes), read back through libhdf5."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_fixtures import H5File
    from graph_framework_amd.output import write_bins
    nx, ny, nz = 3, 4, 5
    rng = np.random.default_rng(3)
    values = rng.standard_normal((nx, ny, nz))
    values[0, 0, 0] = 5e-324
    edges = [np.linspace(-1.0, 2.0, nx + 1), np.linspace(0.0, 1.0, ny + 1), np.linspace(-0.5, 0.5, nz + 1)]
    counts = dict(samples=(1 << 33) + 7, outside=12, skipped=3)
    path = str(tmp_path / "bins.nc")
    write_bins(path, values, *edges, **counts)

    f = H5File(path)
    got = f.read("bins")
    assert got.shape == (nx, ny, nz) and got.tobytes() == values.tobytes()
    for name, want in zip(("xbins", "ybins", "zbins"), edges):
        got = f.read(name)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
    for name, length in (("nx", nx), ("ny", ny), ("nz", nz), ("nxp", nx + 1), ("nyp", ny + 1), ("nzp", nz + 1)):
        assert f.read(name).shape == (length,), name
    f.close()

    lib = _hdf5_reader()
    hid = ctypes.c_int64
    file = lib.H5Fopen(path.encode(), 0, 0)
    assert file >= 0
    assert lib.H5Aexists(file, b"_NCProperties") > 0
    int64 = hid.in_dll(lib, "H5T_NATIVE_INT64_g").value
    for name, want in counts.items():
        attribute = lib.H5Aopen(file, name.encode(), 0)
        assert attribute >= 0, name
        value = ctypes.c_int64()
        assert lib.H5Aread(attribute, int64, ctypes.byref(value)) >= 0 and value.value == want, name
        lib.H5Aclose(attribute)
    dimensions = {}
    for dimid, name in enumerate(("nx", "ny", "nz", "nxp", "nyp", "nzp")):
        dimensions[name] = lib.H5Dopen2(file, name.encode(), 0)
        assert dimensions[name] >= 0 and lib.hl.H5DSis_scale(dimensions[name]) > 0, name
        attribute = lib.H5Aopen(dimensions[name], b"_Netcdf4Dimid", 0)
        value = ctypes.c_int()
        native_int = hid.in_dll(lib, "H5T_NATIVE_INT_g").value
        assert lib.H5Aread(attribute, native_int, ctypes.byref(value)) >= 0 and value.value == dimid, name
        lib.H5Aclose(attribute)
        assert lib.H5Aexists(dimensions[name], b"NAME") > 0
    for name, axes in (("bins", ("nx", "ny", "nz")), ("xbins", ("nxp",)), ("ybins", ("nyp",)), ("zbins", ("nzp",))):
        dataset = lib.H5Dopen2(file, name.encode(), 0)
        assert dataset >= 0, name
        kind = lib.H5Dget_type(dataset)
        assert lib.H5Tget_class(kind) == 1 and lib.H5Tget_size(kind) == 8, name        # H5T_FLOAT, f8
        lib.H5Tclose(kind)
        for axis, dimension in enumerate(axes):
            assert lib.hl.H5DSget_num_scales(dataset, axis) == 1, (name, axis)
            for other, scale in dimensions.items():
                assert (lib.hl.H5DSis_attached(dataset, scale, axis) > 0) == (other == dimension), (name, axis, other)
        lib.H5Dclose(dataset)
    for dataset in dimensions.values():
        lib.H5Dclose(dataset)
    lib.H5Fclose(file)
