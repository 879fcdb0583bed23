"""Records that hold the same bits are merged before an item is cut and written (graph_framework_amd/csrc/merge.hpp,
GFHIP_MERGE, default on), checked on the CPU: the DAG the lowering exports computes the bits of the item as it arrived
on the oracle, the report names the merges that were planted and no others, the assembly statement of a merged item
replays on symbolic values, and GFHIP_MERGE=0 writes the text the lowering wrote before the pass existed.

What is merged: add, sub, mul, fma, div and powi records with the same operation and operands (same order), and
powi(x, p) through its prefix powi(x, p - 1).  What is NOT: sqrt and pow (tests/test_cabi.py counts their sequences
per record), commutative twins and products with -1.0 (the second tier of the design, left out: DESIGN.md section 3).
The device side is tests/test_gpu_merge.py."""
import glob
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import asm_symbolic
import gfir_random
from gfir_random import ADD, CONST, DIV, FMA, MUL, NONE, POWI, SQRT, SUB
from conftest import ROOT, WORKLOADS

#  The kernel texts of solver_kernel_f64 (the pass, the redo kernel) as the commit before merge.hpp wrote them: cache hashes
#  and the SHA-256 of the pass, recorded from a build of that commit.
PARENT_HASHES = (0xc29f21778ef2753a, 0x691d5c1425e9143a)
PARENT_PASS_SHA256 = "4a055c328d20d384f0c47b0fc658bee693c2293f38162465eec750e4132ae0bf"


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def edge_values(real):
    """The operands of tests/test_gpu_division.py: +-0, +-inf, 2^+-600 (2^+-110 in fp32), the largest and the smallest
    normal numbers, subnormal numerators."""
    from test_gpu_division import _operands
    columns = _operands("f64" if real == np.float64 else "f32", tiny_numerators=True)
    return np.unique(bits(np.concatenate([columns[0], columns[2]]))).view(real)


def rays_with_edges(inputs, real, random_rays=256, seed=7, low=-1.0, high=1.0):
    """`random_rays` random rays, then rows in which every input, and rows in which one input, holds an edge value."""
    rng = np.random.default_rng(seed)
    edges = edge_values(real)
    columns = [rng.uniform(low, high, random_rays).astype(real) for _ in range(inputs)]
    everywhere = [edges.copy() for _ in range(inputs)]
    single = [rng.uniform(low, high, edges.size*inputs).astype(real) for _ in range(inputs)]
    for i in range(inputs):
        single[i][i*edges.size:(i + 1)*edges.size] = edges
    return [np.ascontiguousarray(np.concatenate(parts)) for parts in zip(columns, everywhere, single)]


def run_pieces(pieces, columns):
    """The exported pieces of an item, one after the other, on the oracle (as tests/test_cabi.py walks a split item)."""
    from oracle import gfir
    slots = [None]*pieces[0]["slots"]
    outputs = {}
    for piece in pieces:
        item = gfir.Item(piece["gfir"])
        inputs = [columns[state] if state >= 0 else slots[slot].copy()
                  for state, slot in zip(piece["symbol_state"], piece["symbol_slot"])]
        outs, _ = item.run(inputs)
        for value, slot, original in zip(outs, piece["output_slot"], piece["output_original"]):
            if slot >= 0:
                slots[slot] = value
            else:
                outputs[original] = value
    return [outputs[o] for o in sorted(outputs)]


def assert_lowered_dag_computes_the_item(monkeypatch, blob, columns, passes=2):
    """Merge on: the DAG as lowered (exported pieces) against the item as it arrived, every stored array as raw bits."""
    from graph_framework_amd.backend import export_pieces
    from oracle import gfir
    monkeypatch.setenv("GFHIP_MERGE", "1")
    pieces = export_pieces(blob)
    assert pieces, "the item was not exported"
    whole = gfir.Item(blob)
    want_columns = [c.copy() for c in columns]
    got_columns = [c.copy() for c in columns]
    with np.errstate(all="ignore"):
        for _ in range(passes):
            want, _ = whole.run(want_columns)
            got = run_pieces(pieces, got_columns)
            assert len(got) == len(want)
            for a, b in zip(got + got_columns, want + want_columns):
                assert np.array_equal(bits(a), bits(b))
    return pieces


def one_piece(monkeypatch):
    """Knobs under which every item that can be cut is exported: as one piece, or cut by size above 6000 records."""
    monkeypatch.setenv("GFHIP_SEGMENTS", "1")
    monkeypatch.setenv("GFHIP_SEGMENTS_MIN_NODES", "0")


def report_of(capfd, blob):
    """(merged pairs, prefix pairs, counts, kernel texts): the report the lowering prints for the pass of `blob`."""
    from graph_framework_amd.backend import generate_piece_sources
    capfd.readouterr()
    texts = generate_piece_sources(blob)
    err = capfd.readouterr().err
    start = re.search(r"^merge of \w+:", err, re.M).start()
    first, *rest = err[start:].split("\n")
    head = re.match(r"merge of \w+: (\d+) records merged \(add (\d+), sub (\d+), mul (\d+), fma (\d+), div (\d+), powi (\d+)\), (\d+) powi prefixes, "
                    r"(\d+) vector instructions", first)
    lines = []
    for line in rest:
        if not line.startswith("  "):
            break
        lines.append(line)
    merged = {(int(a), int(b)) for a, b in re.findall(r"merged r(\d+) into r(\d+)", "\n".join(lines))}
    prefixed = {(int(a), int(b)) for a, b in re.findall(r"powi r(\d+) from its prefix r(\d+)", "\n".join(lines))}
    counts = dict(zip(("records", "add", "sub", "mul", "fma", "div", "powi", "prefixes", "instructions"), (int(g) for g in head.groups())))
    assert counts["records"] == len(merged) and counts["prefixes"] == len(prefixed)
    return merged, prefixed, counts, texts


REAL_WORKLOADS = sorted(glob.glob(os.path.join(WORKLOADS, "*_f64.gfir")) + glob.glob(os.path.join(WORKLOADS, "*_f32.gfir")))


@pytest.mark.parametrize("path", REAL_WORKLOADS, ids=[os.path.basename(p)[:-5] for p in REAL_WORKLOADS])
def test_shipped_workloads_compute_the_same_bits_merged(monkeypatch, path):
    from graph_framework_amd.backend import export_pieces
    from oracle import gfir
    blob = open(path, "rb").read()
    item = gfir.Item(blob)
    one_piece(monkeypatch)
    if not export_pieces(blob):
#  items the lowering neither cuts nor merges (SAFE_MATH, random draws, index nodes, a single record): the same text
        from graph_framework_amd.backend import generate_piece_sources
        on = generate_piece_sources(blob)
        monkeypatch.setenv("GFHIP_MERGE", "0")
        assert generate_piece_sources(blob) == on
        return
    columns = rays_with_edges(item.num_inputs, item.np_dtype, low=0.25, high=2.5)
    assert_lowered_dag_computes_the_item(monkeypatch, blob, columns)


@pytest.mark.parametrize("nodes", [300, 1500])
def test_fuzz_items_compute_the_same_bits_merged(monkeypatch, nodes):
    blob, _ = gfir_random.random_item(60 + nodes, "f64", 6, nodes, 3, 3)
    one_piece(monkeypatch)
    assert_lowered_dag_computes_the_item(monkeypatch, blob, rays_with_edges(6, np.float64))


def planted_item(dtype="f64", nodes=120, seed=61, name="planted"):
    """A fuzz item with, appended to it, records that hold the same bits as earlier ones.  Returns (GFIR bytes,
    GFIR bytes of the fuzz part alone with the same record numbers, merges, prefixes): `merges` the (record,
    representative) pairs the pass must find among the appended records, `prefixes` the (powi record, prefix record) pairs."""
    rng = np.random.default_rng(seed)
    b = gfir_random.Builder(rng, dtype, 6)
    while len(b.code) < nodes:
        b.grow()
    tail = b.values[-8:]
    base_outputs, base_setters = [tail[0], tail[1]], [(b.squash(tail[2]), 5)]
    base = gfir_random.serialize(b, base_outputs, base_setters, 6, name)

    def raw(op, a=NONE, bb=NONE, c=NONE, aux=0, imm=(0.0, 0.0, 0.0, 0.0)):      # no hash-consing: a record of its own
        b.code.append((op, a, bb, c, aux, tuple(imm)))
        b.bound.append(1.0)
        return len(b.code) - 1

    x, y, z, u = b.inputs[:4]
    shift = raw(CONST, imm=(1.53125, 0.0, 0.0, 0.0))
    minus_one = raw(CONST, imm=(-1.0, 0.0, 0.0, 0.0))
    w = raw(ADD, z, shift)                                  # a base no fuzz record has a power of
    merges, prefixes = set(), set()
#  a duplicated sqrt: both are computed (sqrt is not merged), what reads them is one record
    argument = raw(FMA, x, x, shift)
    s1, s2 = raw(SQRT, argument), raw(SQRT, argument)
    r1, r2 = raw(MUL, s1, y), raw(MUL, s2, y)
    merges.add((r2, r1))
#  a duplicated denominator: one record, one reciprocal; a duplicated quotient
    d1, d2 = raw(FMA, y, y, shift), raw(FMA, y, y, shift)
    merges.add((d2, d1))
    q1, q2, q3 = raw(DIV, x, d1), raw(DIV, u, d2), raw(DIV, x, d2)
    merges.add((q3, q1))
#  powers 2, 3, 4, 5 and 8 of one base next to mul(w, w)
    square = raw(MUL, w, w)
    p2, p3, p4, p5, p8 = (raw(POWI, w, aux=k) for k in (2, 3, 4, 5, 8))
    merges.add((p2, square))
    prefixes.update({(p3, square), (p4, p3), (p5, p4)})     # (the 7th power is no record: the 8th is computed from w)
#  commutative twins and products with -1.0: equal values, but not through this pass
    a1, a2 = raw(ADD, x, u), raw(ADD, u, x)
    m1, m2 = raw(MUL, x, u), raw(MUL, u, x)
    f1, f2 = raw(FMA, x, u, y), raw(FMA, u, x, y)
    negative = raw(MUL, d1, minus_one)
    under_sub, under_div = raw(SUB, x, negative), raw(DIV, u, negative)
    total = raw(ADD, r1, r2)
    for v in (q1, q2, q3, square, p2, p3, p4, p5, a1, a2, m1, m2, f1, f2, under_sub, under_div):
        total = raw(ADD, total, v)
    outputs = base_outputs + [total, p8, negative, s2]
    setters = base_setters + [(b.squash(raw(ADD, q3, p3)), 4)]
    return gfir_random.serialize(b, outputs, setters, 6, name), base, merges, prefixes


def test_planted_merges_are_reported_and_no_others(monkeypatch, capfd, tmp_path):
    blob, base, merges, prefixes = planted_item()
    monkeypatch.setenv("GFHIP_ASM_REPORT", "1")
    monkeypatch.setenv("GFHIP_CACHE_DIR", str(tmp_path))
#  in the order the item arrives in, the report's record numbers are the item's
    monkeypatch.setenv("GFHIP_SCHEDULE", "source")
    one_piece(monkeypatch)
    base_merged, base_prefixed, _, _ = report_of(capfd, base)
    merged, prefixed, counts, _ = report_of(capfd, blob)
    assert merged == base_merged | merges
    assert prefixed == base_prefixed | prefixes
#  a pair costs what its record cost: mul 1, fma 1, div 3 (the reciprocal is shared anyway), powi(w, 2) 1; a prefix saves p - 2
    planted_cost = 1 + 1 + 3 + 1 + (1 + 2 + 3)
    _, _, base_counts, _ = report_of(capfd, base)
    assert counts["instructions"] - base_counts["instructions"] == planted_cost
    assert {k: counts[k] - base_counts[k] for k in ("add", "sub", "mul", "fma", "div", "powi")} == dict(add=0, sub=0, mul=1, fma=1, div=1, powi=1)
    monkeypatch.delenv("GFHIP_SCHEDULE")
    assert_lowered_dag_computes_the_item(monkeypatch, blob, rays_with_edges(6, np.float64))
#  in the pressure-aware order the same records are merged (which of a pair is computed depends on the order)
    scheduled_merged, _, scheduled_counts, _ = report_of(capfd, blob)
    assert len(scheduled_merged) == len(merged) and {k: scheduled_counts[k] for k in ("add", "sub", "mul", "fma", "div")} == \
        {k: counts[k] for k in ("add", "sub", "mul", "fma", "div")}


@pytest.mark.parametrize("pairs", [16, 40])
def test_planted_item_replays(monkeypatch, capfd, tmp_path, pairs):
    """The assembly statement of the planted item on symbolic values, with register pools of 16 and 40 pairs; the DAG it
    is held against is the exported one, which computes the item's bits on the oracle."""
    from graph_framework_amd.backend import export_pieces
    blob, _, merges, _ = planted_item()
    monkeypatch.setenv("GFHIP_ASM", "1")
    monkeypatch.setenv("GFHIP_ASM_MIN_NODES", "0")
    monkeypatch.setenv("GFHIP_ASM_WAVES", "1")
    monkeypatch.setenv("GFHIP_ASM_POOL_LO", str(256 - 2*pairs))
    monkeypatch.setenv("GFHIP_CACHE_DIR", str(tmp_path))
    monkeypatch.setenv("GFHIP_ASM_REPORT", "1")
    merged, _, _, texts = report_of(capfd, blob)
    text = texts[0][0]
    assert "v_rcp_f64" in text, "the item kept the compiled body"
    statement = "\n".join(asm_symbolic.statement_of(text))
    assert len(re.findall(r"; alias r\d+ = r\d+", statement)) == len(merged) >= len(merges)
    assert len(re.findall(r"v_rsq_f64_e32", statement)) >= 2                   # both planted square roots
    pieces = assert_lowered_dag_computes_the_item(monkeypatch, blob, rays_with_edges(6, np.float64))
    assert len(pieces) == 1
    stats = asm_symbolic.replay(pieces[0]["gfir"], text)
    assert stats["definitions"] > 100
    if pairs == 16:
        assert stats["spills"] > 0 and stats["fills"] > 0


def _rk4(monkeypatch, capfd, tmp_path, merge):
    monkeypatch.setenv("GFHIP_MERGE", merge)
    monkeypatch.setenv("GFHIP_ASM_REPORT", "1")
    monkeypatch.delenv("GFHIP_CACHE_DIR", raising=False)
    from graph_framework_amd.backend import generate_piece_sources
    capfd.readouterr()
    pieces = generate_piece_sources(os.path.join(WORKLOADS, "solver_kernel_f64.gfir"))
    return pieces, capfd.readouterr().err


def _vector_lines(text):
    return [line for line in asm_symbolic.statement_of(text) if line.startswith("v_")]


def test_merge_off_writes_the_text_of_the_parent_commit(monkeypatch, capfd, tmp_path):
    pieces, err = _rk4(monkeypatch, capfd, tmp_path, "0")
    assert tuple(h for _, h in pieces) == PARENT_HASHES
    assert hashlib.sha256(pieces[0][0].encode()).hexdigest() == PARENT_PASS_SHA256
    assert "merge of" not in err and not re.search(r"; alias r\d+ = r\d+", pieces[0][0])


def test_rk4_item_loses_exactly_the_instructions_of_its_merges(monkeypatch, capfd, tmp_path):
    """solver_kernel_f64, merge on against GFHIP_MERGE=0: the statement has fewer `v_` lines by exactly the instruction
    cost of the reported merges (57 records, 5 powi prefixes: 66 instructions, 5945 -> 5879), and the same holds for the
    lines of the node sequences alone (the folds of the window check pair up as the registers allow and are counted apart)."""
    off, _ = _rk4(monkeypatch, capfd, tmp_path, "0")
    on, err = _rk4(monkeypatch, capfd, tmp_path, "1")
    head = re.search(r"merge of solver_kernel: (\d+) records merged .*?, (\d+) powi prefixes, (\d+) vector instructions", err)
    records, prefixes, instructions = (int(g) for g in head.groups())
    before, after = _vector_lines(off[0][0]), _vector_lines(on[0][0])
    print("vector lines %d -> %d, report: %d records, %d prefixes, %d instructions" % (len(before), len(after), records, prefixes, instructions))
    assert records == 57 and instructions > 0
    folds = ("v_maximum3_f32", "v_minimum3_f32")
    assert len([v for v in before if not v.startswith(folds)]) - len([v for v in after if not v.startswith(folds)]) == instructions
    assert len(before) - len(after) == instructions
    assert len(re.findall(r"; alias r\d+ = r\d+", on[0][0])) == records


def test_rk4_item_merged_replays_and_defines_every_record(monkeypatch, capfd, tmp_path):
    from graph_framework_amd import generate_source
    from graph_framework_amd.backend import export_pieces
    from test_cabi import _defined_before_use
    monkeypatch.setenv("GFHIP_MERGE", "1")
    path = os.path.join(WORKLOADS, "solver_kernel_f64.gfir")
    on, _ = _rk4(monkeypatch, capfd, tmp_path, "1")
    pieces = export_pieces(path)
    assert len(pieces) == 1
    stats = asm_symbolic.replay(pieces[0]["gfir"], on[0][0])
    assert stats["definitions"] > 3500
#  the compiled body: every record still defined once, before its first use
    monkeypatch.setenv("GFHIP_ASM", "0")
    source, _ = generate_source(path)
    assert _defined_before_use(source, "gfhip_solver_kernel") >= 3878
    assert len(re.findall(r"const real r\d+ = r\d+;", source[:source.index("if (__builtin_expect(bad || zero, 0))")])) >= 57


def test_merge_pass_under_address_and_ub_sanitizers(tmp_path):
    """tests/merge_sanitize.cpp: the pass, and the scheduler, the cut and both writers on what it returns, built with
    -fsanitize=address,undefined over every exported workload and 300 mutated items."""
    binary = str(tmp_path/"merge_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", binary, os.path.join(ROOT, "tests", "merge_sanitize.cpp")])
    workloads = sorted(glob.glob(os.path.join(WORKLOADS, "*.gfir")))
    out = subprocess.run([binary] + workloads + ["--mutate", "8", "300", os.path.join(WORKLOADS, "loss_kernel_kx_f64.gfir")],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("merged")
