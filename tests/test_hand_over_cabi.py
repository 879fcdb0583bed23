"""gfhip_hand_over at the C ABI without a device: the symbol, the entry's layout and the refusals that come before any
device call (include/gf_hip.h)."""
import ctypes

import conftest  # noqa: F401  (puts the repository root on sys.path)


def test_symbol_and_entry_layout():
    from graph_framework_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "gfhip_hand_over")
    assert any(name == "gfhip_hand_over" for name, _, _ in _lib.SYMBOLS)
    entry = _lib.HandOverEntry
    assert ctypes.sizeof(entry) == 24
    assert (entry.to_key.offset, entry.from_key.offset, entry.part.offset, entry.reserved.offset) == (0, 8, 16, 20)


def test_null_arguments_are_refused_before_any_device_call():
    """No context exists here (there is no device to make one on), so all that can be passed is null: every such call
    returns non-zero and says why."""
    from graph_framework_amd import _lib
    lib = _lib.load()
    entries = (_lib.HandOverEntry*1)()
    assert lib.gfhip_hand_over(None, None, entries, 1) != 0
    assert b"null" in lib.gfhip_last_error(None)
    assert lib.gfhip_hand_over(None, None, None, 1) != 0
    assert lib.gfhip_hand_over(None, None, None, 0) != 0
