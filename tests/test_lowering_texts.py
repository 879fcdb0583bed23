"""Every kernel text the lowering writes, held byte for byte to a recording (tests/golden/lowering_texts.json).

Generated text is deterministic and the code-object cache is keyed by the hash of the text: a lowering that writes the
recorded texts runs the recorded code objects.  For every workload under graph_framework_amd/workloads and every
configuration of CONFIGURATIONS one SHA-256 covers, in this order: every (text, hash) of generate_piece_sources, the hash
of generate_source, and every piece of export_pieces (its GFIR bytes, symbol_state, symbol_slot, output_slot,
output_original, slots, pieces); the numbers of texts and of pieces are stored next to it.  The 54 k-record vmec86_*
workloads are lowered under `default` only.

The recording is made from a build of the commit BEFORE a change to the lowering, never from the tree under test:

    python tests/test_lowering_texts.py <root of a built checkout of that commit>

writes the JSON next to this file (without an argument: from this tree).  A change that is meant to keep every text is
wrong wherever a digest differs; the file is not recorded again for it."""
import contextlib
import glob
import hashlib
import json
import os
import struct
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lowering_texts.json")

THREE = {"GFHIP_SEGMENTS": "3", "GFHIP_SEGMENTS_MIN_NODES": "40"}
ONE = {"GFHIP_SEGMENTS": "1", "GFHIP_SEGMENTS_MIN_NODES": "0"}
CONFIGURATIONS = {
    "default": {},
    "MERGE=0": {"GFHIP_MERGE": "0"},
    "ASM=0": {"GFHIP_ASM": "0"},
    "SCHEDULE=source": {"GFHIP_SCHEDULE": "source"},
    "DIVISION=ieee": {"GFHIP_DIVISION": "ieee"},
    "DIVISION=checked": {"GFHIP_DIVISION": "checked"},
    "DIVISION=fast": {"GFHIP_DIVISION": "fast"},
    "park off": {"GFHIP_PARK": "0", "GFHIP_ASM": "0"},
    "park capacity": {"GFHIP_PARK_CAPACITY": "100", "GFHIP_ASM": "0"},
    "size cut": {"GFHIP_SEGMENT_NODES": "1500"},
    "three segments": dict(THREE),
    "three segments, ASM=0": dict(THREE, GFHIP_ASM="0"),
    "three segments, MERGE=0": dict(THREE, GFHIP_MERGE="0"),
    "three segments, source order": dict(THREE, GFHIP_SCHEDULE="source"),
    "one segment": dict(ONE),
    "one segment, ASM=0": dict(ONE, GFHIP_ASM="0"),
    "small assembly": {"GFHIP_ASM_MIN_NODES": "0", "GFHIP_ASM_TRIES": "3", "GFHIP_ASM_WAVES": "1"},
}


def workloads(root, configuration):
    paths = sorted(glob.glob(os.path.join(root, "graph_framework_amd", "workloads", "*.gfir")))
    return [p for p in paths if configuration == "default" or not os.path.basename(p).startswith("vmec86_")]


@contextlib.contextmanager
def environment(variables, cache_directory):
    """Every GFHIP_* variable cleared, then `variables` and GFHIP_CACHE_DIR set; what was there comes back afterwards."""
    saved = {k: v for k, v in os.environ.items() if k.startswith("GFHIP_")}
    for k in saved:
        del os.environ[k]
    os.environ.update(variables, GFHIP_CACHE_DIR=str(cache_directory))
    try:
        yield
    finally:
        for k in [k for k in os.environ if k.startswith("GFHIP_")]:
            del os.environ[k]
        os.environ.update(saved)


def digest(backend, path):
    """{"sha256", "texts", "pieces"} of one workload under the environment as it stands."""
    blob = open(path, "rb").read()
    h = hashlib.sha256()

    def put(data):
        h.update(struct.pack("<Q", len(data)))
        h.update(data)

    texts = backend.generate_piece_sources(blob)
    for text, text_hash in texts:
        put(text.encode())
        put(struct.pack("<Q", text_hash))
    put(struct.pack("<Q", backend.generate_source(blob)[1]))
    pieces = backend.export_pieces(blob)
    for piece in pieces:
        put(piece["gfir"])
        for field in ("symbol_state", "symbol_slot", "output_slot", "output_original"):
            put(struct.pack("<%di" % len(piece[field]), *piece[field]))
        put(struct.pack("<ii", piece["slots"], piece["pieces"]))
    return {"sha256": h.hexdigest(), "texts": len(texts), "pieces": len(pieces)}


def digests(backend, root, configuration, cache_directory):
    with environment(CONFIGURATIONS[configuration], cache_directory):
        return {os.path.basename(p)[:-5]: digest(backend, p) for p in workloads(root, configuration)}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cache_directory(tmp_path_factory):
    return tmp_path_factory.mktemp("lowering_texts_cache")


@pytest.mark.parametrize("configuration", list(CONFIGURATIONS))
def test_every_text_is_the_recorded_one(golden, cache_directory, configuration):
    from graph_framework_amd import backend
    got = digests(backend, ROOT, configuration, cache_directory)
    want = golden[configuration]
    assert sorted(got) == sorted(want)
    different = {name: (got[name], want[name]) for name in got if got[name] != want[name]}
    assert not different, "%d of %d workloads differ under %r: %s" % (len(different), len(got), configuration, sorted(different))


def test_recording_covers_the_matrix(golden):
    assert sorted(golden) == sorted(CONFIGURATIONS)
    assert all(sorted(golden[c]) == [os.path.basename(p)[:-5] for p in workloads(ROOT, c)] for c in CONFIGURATIONS)
    changed = {c: sum(golden[c][name] != golden["default"][name] for name in golden[c]) for c in CONFIGURATIONS}
    print("entries: %d; digests that differ from default: %s" % (sum(len(v) for v in golden.values()), changed))
#  the matrix reaches the branches: each of these knobs changes some text
    assert all(changed[c] > 0 for c in CONFIGURATIONS if c != "default")


def test_cold_and_warm_cache_write_the_same_text(golden, tmp_path):
    """solver_kernel_f64 from an empty cache directory (the order search runs and leaves its seed there, unless the
    package's own kernel cache already holds it), then from the same directory (the stored seed is read back): one
    digest, the recorded one."""
    from graph_framework_amd import _lib, backend
    path = os.path.join(ROOT, "graph_framework_amd", "workloads", "solver_kernel_f64.gfir")
    with environment({}, tmp_path):
        cold = digest(backend, path)
        assert glob.glob(str(tmp_path/"*.order")) or glob.glob(os.path.join(_lib.CACHE_DIR, "*.order")), "the search left no seed"
        warm = digest(backend, path)
    assert cold == warm == golden["default"]["solver_kernel_f64"]


if __name__ == "__main__":
    import tempfile
    root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT
    sys.path.insert(0, root)
    from graph_framework_amd import backend as recorded_backend
    assert os.path.dirname(os.path.dirname(os.path.abspath(recorded_backend.__file__))) == root
    with tempfile.TemporaryDirectory() as scratch:
        recording = {c: digests(recorded_backend, root, c, scratch) for c in CONFIGURATIONS}
    with open(GOLDEN, "w") as f:
        json.dump(recording, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d entries from %s" % (sum(len(v) for v in recording.values()), root))
