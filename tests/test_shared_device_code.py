"""Device code that two HIP libraries must compute alike exists once, in a header both include, and the
Makefile rebuilds every library whose headers change.  Text only: nothing is compiled or loaded here."""
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "onepose_st_amd", "csrc")
INCLUDE = os.path.join(REPO, "include")

# header -> (the files that must include it, the head of every function it is the one home of)
SHARED = {
    "sfm_sample.h": (("loftr_sfm.hip", "sfm_fine.hip"),
                     (r"float rint_t\(float ", r"double rint_t\(double ", r"\bT clip\(T ", r"long long cell_id\(", r"float normalise\(T ",
                      r"f32x4 row4\(", r"f32x4 sample_row\(")),
    "crop_pixel.h": (("prep.hip", "track_crop.hip"), (r"float crop_pixel\(",)),
    "reduce_f64.h": (("postopt.hip", "postopt_lm.hip", "temporal_refine.hip", "pnp_device.hip", "pose_eval.hip", "sfm_triangulate.hip"),
                     (r"double wave_sum\(double ", r"double uniform\(double ", r"void block_sums\(double\* ")),
    "device_loop.h": (("pnp_device.hip", "track_box.hip", "detect_affine.hip", "temporal_refine.hip", "sfm_triangulate.hip"),
                      (r"int clamped_count\(const int\* ", r"uint64_t mix64\(uint64_t ")),
    "postopt_fold.h": (("postopt.hip", "postopt_lm.hip"), (r"void fold_row\(",)),
}


def read(path):
    with open(path) as f:
        return f.read()


def sources():
    return {n: read(os.path.join(CSRC, n)) for n in sorted(os.listdir(CSRC)) if n.endswith((".hip", ".h"))}


@pytest.mark.parametrize("header", sorted(SHARED))
def test_one_definition_and_every_consumer_includes_it(header):
    consumers, heads = SHARED[header]
    texts = sources()
    for name in consumers:
        assert f'#include "{header}"' in texts[name], f"{name} does not include {header}"
    for head in heads:
        found = [(n, m.group(0)) for n, t in texts.items() for m in re.finditer(rf"^[^\n/]*__device__[^\n/]*{head}", t, re.M)]
        assert [n for n, _ in found] == [header], (head, found)


def test_the_sample_and_crop_consumers_keep_no_arithmetic_of_their_own():
    texts = sources()
    for name in ("loftr_sfm.hip", "sfm_fine.hip"):
        assert not re.search(r"\brintf?\(|floorf\(|9\.0e18", texts[name]), name
    for name in ("prep.hip", "track_crop.hip"):
        kernel = texts[name][texts[name].index("void crop_"):]
        kernel = kernel[:kernel.index("\n}\n")]
        assert "crop_pixel(" in kernel and not re.search(r"fmaf\(|floorf\(|rintf\(", kernel), name
    # the mixer's multipliers stand in one file
    assert [n for n, t in texts.items() if "0xBF58476D1CE4E5B9" in t] == ["device_loop.h"]


def makefile_lists():
    """{library: (sources, header list)} from csrc/Makefile: SRCS / HDRS of the main library, <TAG>_SRCS / <TAG>_HDRS of a satellite"""
    mk = read(os.path.join(CSRC, "Makefile"))
    var = {m.group(1): m.group(2).split() for m in re.finditer(r"^(\w+) :?= *(.*)$", mk, re.M)}
    tags = re.findall(r"^\$\(eval \$\(call satellite,([A-Z]+),[a-z]+,\w+\)\)$", mk, re.M)
    assert len(tags) >= 10 and all(f"{t}_SRCS" in var and f"{t}_HDRS" in var for t in tags), tags
    libs = {"main": (var["SRCS"], var["HDRS"])}
    libs.update({t: (var[f"{t}_SRCS"], var[f"{t}_HDRS"]) for t in tags})
    return libs


def quoted_includes(text):
    return [i for i in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, re.M) if i != "build/src_hash.h"]


def find_header(name):
    for root in (CSRC, INCLUDE):
        if os.path.exists(os.path.join(root, name)):
            return os.path.join(root, name)
    raise AssertionError(f"{name}: neither under csrc/ nor under include/")


@pytest.mark.parametrize("lib", sorted(makefile_lists()))
def test_every_included_header_is_a_dependency_of_its_library(lib):
    """an edited header must rebuild every object that includes it, directly or through another header"""
    srcs, hdrs = makefile_lists()[lib]
    listed = {os.path.basename(h) for h in hdrs}
    assert srcs and len(listed) == len(hdrs)
    for src in srcs:
        for inc in quoted_includes(read(os.path.join(CSRC, src))):
            assert os.path.basename(inc) in listed, f"{lib}: {src} includes {inc}, which is not in its header list"
            for inner in quoted_includes(read(find_header(inc))):
                assert os.path.basename(inner) in listed, f"{lib}: {src} includes {inc}, which includes {inner}: not in the header list"


def test_shared_headers_stand_in_both_lists():
    libs = makefile_lists()
    main = {os.path.basename(h) for h in libs["main"][1]}
    assert {"sfm_sample.h", "crop_pixel.h", "reduce_f64.h", "postopt_fold.h"} <= main and "device_loop.h" not in main
    for header in ("sfm_sample.h", "crop_pixel.h", "reduce_f64.h"):
        text = read(os.path.join(CSRC, header))
        assert quoted_includes(text) == [] and sorted(re.findall(r"#include <([^>]+)>", text)) == ["hip/hip_runtime.h", "stdint.h"], header
        assert not re.search(r'extern "C"|getenv|OPHIP_LAUNCH|CAPI_CHECK_LAUNCH|<<<', text), header
        # contraction is switched off inside function bodies only: a file-scope pragma would reach the files that include the header
        lines = text.splitlines()
        for i, line in enumerate(lines):
            assert not line.startswith("#pragma clang fp") or lines[i - 1].rstrip().endswith("{"), (header, i + 1)
