"""Lowering level 1 on the CPU (graph_framework_amd/csrc/options.hpp `level`; merge.hpp, asm_body.hpp).

Level 0 is the lowering as it has always been: its texts are the recorded ones (tests/test_lowering_texts.py), and the
entry points that take a level write them at level 0.  Level 1 changes the assembly statement of a `last` piece and
nothing else; the statement it writes is replayed on symbolic values (tests/asm_symbolic_level1.py) for the three solver
items and for random items with every fold planted in them (tests/level1_items.py), through register pools down to 16
pairs.  The bits are the GPU tests' business (tests/test_gpu_level1.py)."""
import base64
import ctypes
import glob
import hashlib
import json
import os
import re
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                 # (run as a script, to record tests/golden/level1_texts.json)
    sys.path.insert(0, ROOT)

import asm_symbolic
import asm_symbolic_level1
import level1_items
from test_lowering_texts import CONFIGURATIONS, environment

WORKLOADS = os.path.join(ROOT, "graph_framework_amd", "workloads")
GOLDEN = os.path.join(ROOT, "tests", "golden", "level1_texts.json")
SOLVERS = ("solver_kernel_f64", "adaptive_rk4_solver_kernel_f64", "ordinary_wave_solver_kernel_f64")
STATEMENT = re.compile(r'asm volatile\(\n.*?"memory"\);\n', re.S)

#  Vector instructions of the statement of solver_kernel_f64: as the lowering has always written it, and at level 1 (24 mul
#  by -1.0 and 16 gathers of tables derived by -1.0 became modifiers, 8 commutative twins and 3 square roots were merged).
RK4_VECTOR_LEVEL0 = 5879
RK4_VECTOR_LEVEL1 = 5799


def shipped(include_vmec86=False):
    paths = sorted(glob.glob(os.path.join(WORKLOADS, "*.gfir")))
    return [p for p in paths if include_vmec86 or not os.path.basename(p).startswith("vmec86_")]


def vector_instructions(text):
    return sum(1 for line in asm_symbolic.statement_of(text) if line.startswith("v_"))


@pytest.fixture(scope="module")
def cache_directory(tmp_path_factory):
    return tmp_path_factory.mktemp("level1_cache")


def old_piece_sources(lib, blob):
    """[(text, hash)] through gfhip_generate_piece_source, the entry point without a level."""
    pieces = []
    while True:
        text, source_hash = ctypes.c_void_p(), ctypes.c_uint64()
        assert lib.gfhip_generate_piece_source(blob, len(blob), len(pieces), ctypes.byref(text), ctypes.byref(source_hash)) == 0
        if not text:
            return pieces
        pieces.append((ctypes.string_at(text).decode(), source_hash.value))
        lib.gfhip_free_string(text)


def old_export_pieces(lib, blob):
    pieces = []
    while True:
        block, size = ctypes.c_void_p(), ctypes.c_size_t()
        assert lib.gfhip_export_piece(blob, len(blob), len(pieces), ctypes.byref(block), ctypes.byref(size)) == 0
        if not block:
            return pieces
        pieces.append(ctypes.string_at(block, size.value))
        lib.gfhip_free_string(block)


def test_level_0_is_the_entry_points_without_a_level(cache_directory):
    """gfhip_generate_piece_source, gfhip_generate_source and gfhip_export_piece return the bytes of their `_at`
    counterparts at level 0, for every shipped workload (what those bytes are: tests/test_lowering_texts.py), and
    GFHIP_LEVEL=0 brings a caller that asks for level 1 back to them."""
    from graph_framework_amd import _lib, backend
    lib = _lib.load()
    with environment({}, cache_directory):
        for path in shipped(include_vmec86=True):
            blob = open(path, "rb").read()
            assert old_piece_sources(lib, blob) == backend.generate_piece_sources(blob, 0), path
            source_hash = ctypes.c_uint64()
            text = lib.gfhip_generate_source(blob, len(blob), ctypes.byref(source_hash))
            source = ctypes.string_at(text).decode()
            lib.gfhip_free_string(text)
            assert (source, source_hash.value) == backend.generate_source(blob, 0), path
            assert old_export_pieces(lib, blob) == _exported(lib, blob, 0), path
    blob = open(os.path.join(WORKLOADS, "solver_kernel_f64.gfir"), "rb").read()
    with environment({}, cache_directory):
        level0, level1 = backend.generate_piece_sources(blob, 0), backend.generate_piece_sources(blob, 1)
    with environment({"GFHIP_LEVEL": "0"}, cache_directory):
        assert backend.generate_piece_sources(blob, 1) == level0
    with environment({"GFHIP_LEVEL": "1"}, cache_directory):
        assert backend.generate_piece_sources(blob, 0) == level1
    assert level0 != level1


def _exported(lib, blob, level):
    pieces = []
    while True:
        block, size = ctypes.c_void_p(), ctypes.c_size_t()
        assert lib.gfhip_export_piece_at(blob, len(blob), len(pieces), ctypes.byref(block), ctypes.byref(size), level) == 0
        if not block:
            return pieces
        pieces.append(ctypes.string_at(block, size.value))
        lib.gfhip_free_string(block)


@pytest.mark.parametrize("configuration", ["default", "ASM=0", "MERGE=0", "DIVISION=ieee", "three segments", "one segment", "small assembly"])
def test_level_1_changes_the_assembly_statement_and_nothing_else(cache_directory, configuration):
    """Piece by piece: the same number of texts, the same pieces as data, and texts that are equal once the assembly
    statement is cut out of both.  A text without a statement — a compiled body, an item the writer refuses, a `middle`
    piece, the redo kernel — is the same text with the same hash."""
    from graph_framework_amd import _lib, backend
    lib = _lib.load()
    changed = []
    with environment(CONFIGURATIONS[configuration], cache_directory):
        for path in shipped():
            blob = open(path, "rb").read()
            level0, level1 = backend.generate_piece_sources(blob, 0), backend.generate_piece_sources(blob, 1)
            assert len(level0) == len(level1), path
            assert _exported(lib, blob, 0) == _exported(lib, blob, 1), path
            for (text0, hash0), (text1, hash1) in zip(level0, level1):
                if "asm volatile(\n" not in text0:
                    assert (text0, hash0) == (text1, hash1), path
                    continue
                assert STATEMENT.sub("STATEMENT\n", text0) == STATEMENT.sub("STATEMENT\n", text1), path
                assert len(STATEMENT.findall(text1)) == len(STATEMENT.findall(text0)) == 1, path
                if text0 != text1:
                    assert hash0 != hash1
                    changed.append(os.path.basename(path))
    print(configuration, "level 1 changes", sorted(set(changed)))
    if configuration in ("ASM=0", "DIVISION=ieee"):
        assert not changed
    elif configuration in ("default", "MERGE=0"):
        assert "solver_kernel_f64.gfir" in changed
    else:
#  (the last third of the RK4 step does not fit the registers at level 0 and keeps the compiled body at both levels)
        assert changed


def lowered(blob, environment_variables, cache_directory, level=1):
    """(piece as GFIR, kernel text) of the item's first piece at `level`, in a child process (the lowering reads its options
    from the environment)."""
    script = ("import sys, json, base64; sys.path.insert(0, %r)\n"
              "from graph_framework_amd.backend import generate_piece_sources, export_pieces\n"
              "blob = base64.b64decode(sys.stdin.read())\n"
              "print(json.dumps([base64.b64encode(export_pieces(blob, %d)[0]['gfir']).decode(), generate_piece_sources(blob, %d)[0][0]]))"
              % (ROOT, level, level))
    env = {k: v for k, v in os.environ.items() if not k.startswith("GFHIP_")}
    env.update(environment_variables, GFHIP_CACHE_DIR=str(cache_directory))
    out = subprocess.run([sys.executable, "-c", script], env=env, input=base64.b64encode(blob).decode(), capture_output=True, text=True, check=True)
    piece, text = json.loads(out.stdout)
    return base64.b64decode(piece), text


@pytest.mark.parametrize("name", SOLVERS)
def test_solver_items_replay_at_level_1(cache_directory, name):
    blob = open(os.path.join(WORKLOADS, name + ".gfir"), "rb").read()
    piece, text = lowered(blob, {}, cache_directory)
    stats = asm_symbolic_level1.replay(piece, text)
    assert stats["definitions"] > 1500 and stats["aliases"] > 300
    _, text0 = lowered(blob, {}, cache_directory, level=0)
    assert vector_instructions(text) < vector_instructions(text0)
#  the folds are there to be checked: the level-0 replay, which knows none of them, does not accept this statement
    with pytest.raises(asm_symbolic.ReplayError):
        asm_symbolic.replay(piece, text)
    if name == "solver_kernel_f64":
        assert stats["folded_gathers"] == 16
        assert vector_instructions(text0) == RK4_VECTOR_LEVEL0
        assert vector_instructions(text) == RK4_VECTOR_LEVEL1 < RK4_VECTOR_LEVEL0
        assert len(re.findall(r"v_rsq_f64_e32", text0)) - len(re.findall(r"v_rsq_f64_e32", text)) == 3


PLANTED_CASES = [  # seed, inputs, nodes, first register of the pool, LDS budget of the staged tables
    (61, 6, 200, 64, 65536), (71, 6, 150, 224, 65536), (73, 6, 150, 224, 0), (77, 6, 200, 224, 0), (62, 6, 350, 200, 65536),
    (63, 8, 500, 160, 0), (64, 8, 700, 64, 0), (65, 5, 400, 208, 65536), (66, 8, 600, 128, 0), (67, 3, 250, 216, 65536),
]


@pytest.mark.parametrize("seed,inputs,nodes,pool,budget", PLANTED_CASES, ids=["%d-nodes-pool-%d-lds-%d" % c[2:] for c in PLANTED_CASES])
def test_planted_items_replay_at_level_1(cache_directory, seed, inputs, nodes, pool, budget):
    """Random items with sign records, swapped twins, second square roots and gathers of negated and of +-0.5 tables
    planted in them; pools down to 16 register pairs (first register 224), where nearly every value goes through LDS."""
    blob, planted = level1_items.planted_item(seed, inputs, nodes)
    assert planted["sign"] and planted["swapped"] and planted["flipped"] + planted["halves"]
    knobs = dict(GFHIP_ASM_MIN_NODES="0", GFHIP_ASM_POOL_LO=str(pool), GFHIP_LDS_BUDGET=str(budget), GFHIP_ASM_WAVES="1")
    piece, text = lowered(blob, knobs, cache_directory)
    assert "v_rcp_f64" in text, "the item kept the compiled body"
    stats = asm_symbolic_level1.replay(piece, text)
    _, text0 = lowered(blob, knobs, cache_directory, level=0)
    saved = vector_instructions(text0) - vector_instructions(text)
    print(planted, stats, "vector instructions saved:", saved)
    assert saved > 0
    assert len(re.findall(r"; alias r\d+ = -", text)) > 0
    if pool > 64:
        assert stats["spills"] > 0 and stats["fills"] > 0


def test_random_items_replay_at_level_1(cache_directory):
    """Items of tests/gfir_random.py as they come (what tests/test_asm_body.py replays at level 0)."""
    import gfir_random
    for seed, inputs, nodes, pool in ((42, 6, 150, 224), (47, 8, 500, 160)):
        blob, _ = gfir_random.random_item(seed, "f64", inputs, nodes, 3, 3)
        piece, text = lowered(blob, dict(GFHIP_ASM_MIN_NODES="0", GFHIP_ASM_POOL_LO=str(pool), GFHIP_ASM_WAVES="1"), cache_directory)
        assert asm_symbolic_level1.replay(piece, text)["definitions"] >= nodes//2


def test_corrupted_level_1_statements_are_caught(cache_directory):
    """The level-1 replay is not vacuous: a `neg` modifier dropped from a use of a folded sign record fails it, and so
    does the name of a merged square root that points at another record."""
    blob = open(os.path.join(WORKLOADS, "solver_kernel_f64.gfir"), "rb").read()
    piece, text = lowered(blob, {}, cache_directory)
    asm_symbolic_level1.replay(piece, text)
    lines = text.split("\n")
    item = asm_symbolic.parse(piece)
    ins = item["ins"]
#  a quotient whose numerator is a folded sign record (most of the RK4 step's are): q = n*r is the first instruction of
#  its sequence, two lines above the one that defines the quotient
    folded = [int(m.group(1)) for m in (re.search(r'"; alias r(\d+) = -r\d+\\n"', line) for line in lines) if m]
    assert folded
    users = [k for k in range(len(ins)) if int(ins["op"][k]) == asm_symbolic.OPS["DIV"] and int(ins["a"][k]) in folded]
    defines = {int(m.group(1)): k for k, m in ((k, re.search(r'; def r(\d+)\\n"$', line)) for k, line in enumerate(lines)) if m}
    target = next(defines[u] - 2 for u in users if u in defines and re.search(r'"v_mul_f64 v\[\d+:\d+\], -v\[', lines[defines[u] - 2]))
    broken = lines[target].replace(", -v[", ", v[", 1)
    with pytest.raises(asm_symbolic.ReplayError):
        asm_symbolic_level1.replay(piece, "\n".join(lines[:target] + [broken] + lines[target + 1:]))
#  the three square roots merged at level 1: `; alias rJ = rI` with both records SQRT
    roots = [(k, int(m.group(1)), int(m.group(2))) for k, m in ((k, re.search(r'"; alias r(\d+) = r(\d+)\\n"', line)) for k, line in enumerate(lines))
             if m and int(ins["op"][int(m.group(1))]) == asm_symbolic.OPS["SQRT"]]
    assert len(roots) == 3
    k, record, representative = roots[-1]
    other = next(r for _, _, r in roots if r != representative and r < record)       # an earlier square root, but another one
    broken = lines[k].replace("= r%d\\n" % representative, "= r%d\\n" % other)
    assert broken != lines[k]
    with pytest.raises(asm_symbolic.ReplayError):
        asm_symbolic_level1.replay(piece, "\n".join(lines[:k] + [broken] + lines[k + 1:]))


def level1_digests(cache_directory):
    """{workload: sha256 over every (text, hash) of its pieces at level 1} for the workloads whose level-1 texts differ
    from level 0, under the default options."""
    from graph_framework_amd import backend
    out = {}
    with environment({}, cache_directory):
        for path in shipped():
            blob = open(path, "rb").read()
            level1 = backend.generate_piece_sources(blob, 1)
            if level1 == backend.generate_piece_sources(blob, 0):
                continue
            h = hashlib.sha256()
            for text, text_hash in level1:
                h.update(struct.pack("<Q", len(text.encode())))
                h.update(text.encode())
                h.update(struct.pack("<Q", text_hash))
            out[os.path.basename(path)[:-5]] = {"sha256": h.hexdigest(), "texts": len(level1),
                                                "vector_instructions": vector_instructions(level1[0][0])}
    return out


def test_level_1_texts_are_the_recorded_ones(cache_directory):
    """tests/golden/level1_texts.json: recorded from the build whose level-1 kernels passed tests/test_gpu_level1.py
    (`python tests/test_level1.py` writes it).  A change that is meant to keep the level-1 code objects keeps these."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert level1_digests(cache_directory) == golden
    assert golden["solver_kernel_f64"]["vector_instructions"] == RK4_VECTOR_LEVEL1


def test_level_1_under_address_and_ub_sanitizers(tmp_path):
    """tests/level1_sanitize.cpp: plan_item() at level 1, and the level-1 merge on its own, built with
    -fsanitize=address,undefined, over every exported workload and 132 mutated items."""
    binary = str(tmp_path/"level1_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", binary, os.path.join(ROOT, "tests", "level1_sanitize.cpp")])
    workloads = sorted(glob.glob(os.path.join(WORKLOADS, "*.gfir")))
    out = subprocess.run([binary] + workloads + ["--mutate", "9", "120", os.path.join(WORKLOADS, "loss_kernel_kx_f64.gfir"),
                                                 "--mutate", "10", "12", os.path.join(WORKLOADS, "ordinary_wave_solver_kernel_f64.gfir")],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("planned")


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as scratch:
        recording = level1_digests(scratch)
    with open(GOLDEN, "w") as f:
        json.dump(recording, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d entries" % len(recording))
