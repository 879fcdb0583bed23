"""CPU tests of the table lowering (graph_framework_amd/csrc/tables.hpp) on the planted tables of
tests/planted_tables.py: the numpy model of a gather against the oracle, the compaction's invariant — a derived table
is k*parent bit pattern for bit pattern, the sign of a zero included — the decisions that are certain, and the packs.
The device side is tests/test_gpu_tables.py."""
import re
import struct

import numpy as np
import pytest

import planted_tables
from planted_tables import COLS, DERIVED, LENGTHS, REAL, ROWS, STORED, differing, same_bits

DTYPES = ["f64", "f32"]


@pytest.fixture(scope="module")
def lib():
    from graph_framework_amd import build, _lib
    build.build_library()
    return _lib.load()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("probe", ["gather", "index"])
def test_numpy_model_and_oracle_agree_on_every_lane(probe, dtype):
    """oracle/gfir_interp.c's index against an independent restatement, before the GPU is held to either: both probes,
    two passes, every output and every input after the setters."""
    from oracle import gfir
    columns = planted_tables.probe_arguments(dtype)
    if probe == "gather":
        item = planted_tables.gather_probe(dtype)
    else:
        item, buffers = planted_tables.index_probe(dtype, columns[0].size)
        columns += buffers
    oracle_item = gfir.Item(item.blob)
    assert oracle_item.num_instructions == item.records < 100
    modelled, expected = [c.copy() for c in columns], [c.copy() for c in columns]
    with np.errstate(all="ignore"):
        for launch in range(2):
            want, _ = oracle_item.run(expected)
            got = item.model(modelled)
            assert len(got) == len(want)
            for key, a, b in zip(item.in_keys + item.out_keys, modelled + got, expected + want):
                assert same_bits(a, b), (key, launch, differing(a, b)[:8])
#  the planted lanes do reach both ends, the NaN lane and every cell of the longest table
    x = columns[0]
    cells = planted_tables.cell(REAL[dtype], x, *planted_tables.ARGUMENTS[33], 33)
    assert set(cells) == set(range(33)) and np.isnan(x).any() and np.isinf(x).any()


def _multiplies(dtype, compiled, assembly=None):
    """{child table: (factor, parent table)} from the lines `const real cG_T = K*cG_P;` of a compiled body or from the
    annotations `; def cG_T = cG_P * <bits of K>` of an assembly body."""
    found = {}
    if assembly is None:
        for child, factor, parent in re.findall(r"const real c\d+_(\d+) = (\S+)\*c\d+_(\d+);", compiled):
            found.setdefault(int(child), set()).add((float.fromhex(factor.rstrip("f")), int(parent)))
    else:
        for child, parent, bits in re.findall(r"; def c\d+_(\d+) = c\d+_(\d+) \* (\d+)", assembly):
            found.setdefault(int(child), set()).add((struct.unpack("<d", struct.pack("<Q", int(bits)))[0], int(parent)))
    assert all(len(v) == 1 for v in found.values())                    # every body of the text multiplies the same pairs
    return {child: next(iter(v)) for child, v in found.items()}


def _hold_invariant(dtype, tables, derived):
    """fl(k*parent) in the item's precision has the child's bit pattern in every cell; chains as the device computes
    them, k_j*(k_i*root)."""
    real = REAL[dtype]

    def value(t):
        if t not in derived:
            return tables[t][1].astype(real)
        k, parent = derived[t]
        assert real(k) == k                                            # the factor is a value of the item's precision
        with np.errstate(all="ignore"):
            return real(k)*value(parent)

    for t in derived:
        want = tables[t][1].astype(real)
        assert not np.isnan(want).any(), tables[t][0]
        assert same_bits(value(t), want), (tables[t][0], tables[derived[t][1]][0], derived[t][0], differing(value(t), want))


def _root(derived, t):
    while t in derived:
        t = derived[t][1]
    return t


@pytest.mark.parametrize("dtype", DTYPES)
def test_derived_tables_have_the_bits_of_their_cells(lib, monkeypatch, dtype):
    from graph_framework_amd import generate_source
    from graph_framework_amd.backend import generate_piece_sources
    tables = planted_tables.planted_tables(dtype)
    probe = planted_tables.gather_probe(dtype)
    monkeypatch.setenv("GFHIP_ASM", "0")
    derived = _multiplies(dtype, generate_source(probe.blob)[0])
    assert len(derived) >= 4*len(LENGTHS) + 1
    _hold_invariant(dtype, tables, derived)
    if dtype == "f64":
#  the assembly body's multiplies (its table numbers are those of the piece the kernel is lowered from, whose tables
#  come in another order: other parents, the same invariant)
        from graph_framework_amd.backend import export_pieces
        from oracle.gfir_to_c import parse
        monkeypatch.setenv("GFHIP_ASM", "1")
        monkeypatch.setenv("GFHIP_ASM_MIN_NODES", "0")
        text = generate_piece_sources(probe.blob)[0][0]
        assert "v_cvt_u32_f64" in text
        multiplied = _multiplies(dtype, None, text)
        assert len(multiplied) >= 4*len(LENGTHS) + 1
        piece = parse(export_pieces(probe.blob)[0]["gfir"])["tables"]
        _hold_invariant(dtype, [("table %d of the piece" % t, np.asarray(entry[2])) for t, entry in enumerate(piece)], multiplied)


@pytest.mark.parametrize("dtype", DTYPES)
def test_decisions_that_are_certain(lib, monkeypatch, dtype):
    """What the compaction must and must not derive whatever else it finds: a multiple whose zeros carry the product's
    signs is derived; the same table with the parent's zero signs, a multiple one ulp off in one cell, tables of zeros
    only and tables with an infinity or a NaN are stored; of 3*c and c one is stored; a chain has one stored root."""
    from graph_framework_amd import generate_source
    names = [name for name, _ in planted_tables.planted_tables(dtype)]
    number = {name: t for t, name in enumerate(names)}
    monkeypatch.setenv("GFHIP_ASM", "0")
    derived = _multiplies(dtype, generate_source(planted_tables.gather_probe(dtype).blob)[0])
    reparented = 0
    for length in LENGTHS:
        def table(name):
            return number["%s_%d" % (name, length)]
        for child, (parent, k) in DERIVED.items():
            assert derived.get(table(child)) == (k, table(parent)), (child, length)
        for name in STORED:
            assert table(name) not in derived, (name, length, derived.get(table(name)))
        three_c, c = table("three_c"), table("c")
        assert (three_c in derived) != (c in derived) and _root(derived, three_c) == _root(derived, c)
        assert _root(derived, table("minus_two_c")) == _root(derived, table("back")) == _root(derived, c)
        reparented += sum(parent > child for child, (_, parent) in derived.items())
    assert reparented >= 1                                              # the second pass did derive from a later table
    assert derived[number["multiple_%dx%d" % (ROWS, COLS)]] == (-4.0, number["base_%dx%d" % (ROWS, COLS)])
    monkeypatch.setenv("GFHIP_COMPACT_TABLES", "0")
    assert not _multiplies(dtype, generate_source(planted_tables.gather_probe(dtype).blob)[0])


CASES = {"negative_factor": ([0.0, 1.0, 0.5, -0.25], [0.0, -4.0, -2.0, 1.0]),         # -4*(+0) is -0: stored +0
         "positive_factor": ([0.0, 1.0, 0.5, -0.25], [-0.0, 3.0, 1.5, -0.75])}       # 3*(+0) is +0: stored -0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_a_zero_of_the_other_sign_keeps_a_table_stored(lib, monkeypatch, case, dtype):
    """Two four-cell tables that are multiples of one another in every cell but a zero, whose sign is not the product's:
    `k*from[c] == to[c]` holds throughout, the bit patterns differ, and a gather of the second table stores that zero."""
    from graph_framework_amd import generate_source
    from test_gpu_generic import Item, INPUT, GATHER1
    it = Item(dtype, False, ["x"], name="zero_sign")
    x = it.emit(INPUT, a=0)
    it.tables = [np.array(cells).reshape(1, 4) for cells in CASES[case]]
    blob = it.blob([it.emit(GATHER1, x, aux=t, imm=(0.25, 0.0, 0.0, 0.0)) for t in range(2)], [])
    monkeypatch.setenv("GFHIP_ASM", "0")
    derived = _multiplies(dtype, generate_source(blob)[0])
    _hold_invariant(dtype, [("table %d" % t, data) for t, data in enumerate(it.tables)], derived)
    assert not derived


def _packs(source):
    """{pack: (base name, stride, {table: column})} from the text of a compiled body."""
    groups = {}
    for group, base, pack, stride in re.findall(r"const real \*const g(\d+) = (lds|pack)(\d+) \+ .*\)\*(\d+)u\);", source):
        groups.setdefault(int(group), set()).add((base, int(pack), int(stride)))
    assert groups and all(len(v) == 1 for v in groups.values())
    packs = {}
    for group, table, loaded, column in re.findall(r"const real c(\d+)_(\d+) = g(\d+)\[(\d+)u\];", source):
        assert group == loaded
        base, pack, stride = next(iter(groups[int(group)]))
        entry = packs.setdefault(pack, (base, stride, {}))
        assert entry[:2] == (base, stride) and entry[2].setdefault(int(table), int(column)) == int(column)
    return packs


@pytest.mark.parametrize("dtype", DTYPES)
def test_packs_and_their_staging(lib, monkeypatch, dtype):
    """One pack per shape, a column of its own below an even stride for every stored table, and LDS staging of the
    smallest packs that fit GFHIP_LDS_BUDGET."""
    from graph_framework_amd import generate_source
    tables = planted_tables.planted_tables(dtype)
    blob = planted_tables.gather_probe(dtype).blob
    monkeypatch.setenv("GFHIP_ASM", "0")
    source = generate_source(blob)[0]
    derived = _multiplies(dtype, source)
    packs = _packs(source)
    shapes = [(1, length) for length in LENGTHS] + [(ROWS, COLS)]
    assert len(packs) == len(shapes)
    size = {}
    for pack, (base, stride, columns) in packs.items():
        shape = {tables[t][1].shape for t in columns}
        assert len(shape) == 1
        stored = [t for t, (_, data) in enumerate(tables) if data.shape in shape and t not in derived]
        assert sorted(columns) == stored                                # every stored table of the shape, and only those
        assert sorted(columns.values()) == list(range(len(stored)))     # distinct columns, all below the stride
        assert stride % 2 == 0 and len(stored) <= stride <= len(stored) + 1
        assert base == "lds"                                            # the default budget holds all of them
        rows, cols = shape.pop()
        size[pack] = rows*cols*stride*np.dtype(REAL[dtype]).itemsize
    assert any(len(columns) % 2 for _, _, columns in packs.values())    # a pad column exists
#  A budget that takes the two smallest packs and not the third (a staged pack takes a multiple of 16 bytes).
    order = sorted(size, key=lambda p: size[p])
    assert size[order[1]] < size[order[2]]
    budget = (size[order[0]] + 15)//16*16 + size[order[1]]
    monkeypatch.setenv("GFHIP_LDS_BUDGET", str(budget))
    split = _packs(generate_source(blob)[0])
    assert {p: split[p][0] for p in split} == {p: ("lds" if p in order[:2] else "pack") for p in size}
    assert all(split[p][1:] == packs[p][1:] for p in packs)             # where a pack lies changes nothing in it
    monkeypatch.setenv("GFHIP_LDS_BUDGET", str(budget - 1))
    assert sorted(p for p, entry in _packs(generate_source(blob)[0]).items() if entry[0] == "lds") == [order[0]]
    monkeypatch.setenv("GFHIP_LDS_BUDGET", "0")
    assert all(entry[0] == "pack" for entry in _packs(generate_source(blob)[0]).values())


def staging_budget(dtype):
    """A GFHIP_LDS_BUDGET under which the probe's smaller packs are staged in LDS and its larger ones are read from
    global memory (tests/test_gpu_tables.py): the bytes of the two smallest packs, from the text of the default
    lowering."""
    from graph_framework_amd import generate_source
    tables = planted_tables.planted_tables(dtype)
    packs = _packs(generate_source(planted_tables.gather_probe(dtype).blob)[0])
    sizes = sorted(tables[next(iter(columns))][1].size*stride*np.dtype(REAL[dtype]).itemsize
                   for _, stride, columns in packs.values())
    return (sizes[0] + 15)//16*16 + sizes[1]
