"""The knob and the counters of proj320s_kernel (csrc/proj320_stream.hip) through the C ABI, without a GPU: IDF_TUNE_PROJ_ROW = 9 takes
0 / 1 and returns the previous value, IDF_STAT_PROJ_ROW_LAUNCHES = 8 is a known counter, and the header, the Python constants and the
build list name the same things."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_knob_and_counter():
    from instancediffusion_amd import _lib
    lib = _lib.load()
    assert _lib.IDF_TUNE_PROJ_ROW == 9 and lib.idf_set_tuning(8, 0) == -1 and _lib.IDF_STAT_PROJ_ROW_LAUNCHES == 8 and _lib.IDF_STAT_PROJ_ROW_MIN_M == 9
    assert lib.idf_abi_version() == 5
    n0 = lib.idf_get_stat(_lib.IDF_STAT_PROJ_ROW_LAUNCHES)
    assert n0 >= 0                                            # a known counter (whatever this process has launched so far)
    assert lib.idf_set_tuning(_lib.IDF_TUNE_PROJ_ROW, 2) == -1 and lib.idf_set_tuning(_lib.IDF_TUNE_PROJ_ROW, -1) == -1
    prev = lib.idf_set_tuning(_lib.IDF_TUNE_PROJ_ROW, 0)
    assert prev == (0 if os.environ.get("IDF_PROJ_ROW", "1")[:1] == "0" else 1)
    assert lib.idf_set_tuning(_lib.IDF_TUNE_PROJ_ROW, prev) == 0
    # (stat 10 is IDF_STAT_ATTN_RES_LAUNCHES since the attention edge tests; 11 is the first unknown id)
    assert lib.idf_get_stat(11) == -1 and lib.idf_get_stat(_lib.IDF_STAT_ATTN_RES_LAUNCHES) >= 0
    assert lib.idf_get_stat(_lib.IDF_STAT_PROJ_ROW_LAUNCHES) == n0                                   # the knob calls launch nothing


def test_header_and_build_list_agree():
    hdr = open(os.path.join(REPO, "include", "idf.h")).read()
    assert re.search(r"IDF_TUNE_PROJ_ROW\s*=\s*9\b", hdr) and re.search(r"IDF_STAT_PROJ_ROW_LAUNCHES\s*=\s*8\b", hdr)
    assert re.search(r"IDF_STAT_PROJ_ROW_MIN_M\s*=\s*9\b", hdr) and re.search(r"#define IDF_ABI_VERSION 5\b", hdr)
    build = open(os.path.join(REPO, "instancediffusion_amd", "csrc", "build.sh")).read()
    assert re.search(r"for f in [^;]*\bproj320_stream\b", build)
    assert os.path.exists(os.path.join(REPO, "instancediffusion_amd", "csrc", "proj320_stream.hip"))
