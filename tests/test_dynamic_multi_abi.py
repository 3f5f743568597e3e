"""CPU suite of the many-sequence colour entry: include/svo.h declares svo_track_multi_step_bgr_dev, the library exports it, the
binding has its method, and the ABI version is unchanged (the entry is a backward-compatible addition).  No GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_colour_step():
    txt = open(os.path.join(ROOT, "include", "svo.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+svo_track_multi_step_bgr_dev\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/svo.h must declare svo_track_multi_step_bgr_dev"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 7 and args[0].startswith("svo_ctx*") and "svo_boxes_dev" in args[5] and "svo_track_result" in args[6]
    gray = re.search(r"\bint\s+svo_track_multi_step_dev\s*\(([^)]*)\)\s*;", txt)
    assert gray and len(gray.group(1).split(",")) == 7


def test_library_exports_it_and_the_abi_version_stays(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    assert hasattr(lib, "svo_track_multi_step_bgr_dev")
    assert lib.svo_abi_version() == 8
    # (argument checks come before any device is touched)
    assert lib.svo_track_multi_step_bgr_dev(None, None, None, 0, 1, None, None) == -1


def test_binding_has_the_method(pkg):
    assert "svo_track_multi_step_bgr_dev" in pkg.ABI_SYMBOLS
    assert callable(getattr(pkg.Svo, "track_multi_step_bgr_dev"))
    assert callable(getattr(pkg.Svo, "track_dynamic_out"))
