"""CPU-only checks of lthip_store (the set of chunk hashes a store already holds) and of the sessions' entry points that consult it:
every name is declared in include/longtail_hip.h and exported by both builds, the gfx950 code object holds the table's kernels, the
binding and the header agree on the interface version, and every call refuses a NULL store / session without a GPU."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from tests.test_abi import declared_symbols

STORE_SYMBOLS = ["lthip_store_create", "lthip_store_destroy", "lthip_store_add", "lthip_store_add_index", "lthip_store_find", "lthip_store_added",
                 "lthip_store_distinct", "lthip_store_grown"]
SESSION_SYMBOLS = ["lthip_ingest_stream_set_store", "lthip_ingest_stream_store_stats", "lthip_ingest_set_store", "lthip_ingest_store_stats"]
STORE_KERNELS = ["k_store_clear", "k_store_insert", "k_store_find", "k_store_reinsert", "k_ing_local_hashes", "k_ing_known_stats"]


def test_entry_points_are_declared_and_exported(hiplib):
    declared = declared_symbols()
    assert set(STORE_SYMBOLS + SESSION_SYMBOLS) <= set(declared)
    assert not [n for n in STORE_SYMBOLS + SESSION_SYMBOLS if not hasattr(hiplib.dll, n)]
    from longtail_amd.lib import ABLATIONS_LIB_PATH

    if ABLATIONS_LIB_PATH.exists():
        abl = C.CDLL(str(ABLATIONS_LIB_PATH))
        assert not [n for n in STORE_SYMBOLS + SESSION_SYMBOLS if not hasattr(abl, n)]


def test_code_object_holds_the_store_kernels(hiplib):
    text = subprocess.run(["strings", "-a", str(hiplib.path)], capture_output=True, text=True, check=True).stdout
    for k in STORE_KERNELS:
        assert k in text, k
    assert "amdgcn-amd-amdhsa--gfx950" in text


def test_interface_version_is_4_everywhere(hiplib):
    from longtail_amd.lib import ABI_VERSION

    root = Path(__file__).resolve().parent.parent
    header = (root / "include" / "longtail_hip.h").read_text()
    assert int(re.search(r"#define LTHIP_ABI_VERSION (\d+)", header).group(1)) == ABI_VERSION == hiplib.dll.lthip_abi_version() == 4
    assert "LTHIP_ABI_VERSION is 4" in (root / "INTEGRATION.md").read_text()


def test_null_store_or_session_is_refused(hiplib):
    d = hiplib.dll
    out, n = C.c_void_p(), C.c_uint64(7)
    assert d.lthip_store_create(None, 0, C.byref(out)) != 0 and not out.value
    assert d.lthip_store_add(None, 0, None) != 0
    assert d.lthip_store_add_index(None, None, 0) != 0
    assert d.lthip_store_find(None, 0, None, None, None) != 0
    assert d.lthip_store_distinct(None, C.byref(n)) != 0 and n.value == 7
    assert d.lthip_store_added(None) == 0 and d.lthip_store_grown(None) == 0
    d.lthip_store_destroy(None)
    assert d.lthip_ingest_stream_set_store(None, None) != 0
    assert d.lthip_ingest_stream_store_stats(None, C.byref(n), C.byref(n)) != 0
    assert d.lthip_ingest_set_store(None, None) != 0
    assert d.lthip_ingest_store_stats(None, C.byref(n), C.byref(n)) != 0


def test_close_leaves_a_store_alone_once_its_context_is_closed():
    """lthip_store_destroy reads its context (device, stream).  Context.close() deletes it, so a Store that is closed -- or collected --
    after its context must not reach the library again; with a live context it does, once."""
    from longtail_amd.lib import Store

    class Dll:
        def __init__(self):
            self.calls = []

        def lthip_store_destroy(self, h):
            self.calls.append(h)

    class Ctx:
        def __init__(self, h):
            self.h, self.lib = h, type("Lib", (), {})()
            self.lib.dll = Dll()

    dead, live = Ctx(None), Ctx(1234)
    for ctx in (dead, live):
        obj = Store.__new__(Store)
        obj.ctx, obj.h = ctx, 77
        obj.close()
        assert obj.h is None
        obj.close()
        del obj
    assert dead.lib.dll.calls == [] and live.lib.dll.calls == [77]
