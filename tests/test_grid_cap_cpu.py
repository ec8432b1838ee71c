"""csrc/idc_grid.h without a device: tools/grid_selftest.cpp (the clamp, the test hook that can only lower a grid, the per-tag record), built
here without a sanitizer (`make grid_selftest SAN=1` is the sanitizer build, for a CPU machine) -- and a reading of csrc/*.hip: every tag of
the header's list is handed to grid_blocks at exactly one launch site, and no launch takes its grid from a `x < CONST ? x : CONST` of its own."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "interactive_deep_colorization_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

TAGS = ["head", "softmax_nchw", "dist313", "lab_post", "pcie_copy", "upsample_lab2rgb", "global_stats", "ingest_rgb", "fullres_rgb",
        "batch_prologue", "batch_fullres_rgb", "ragged_prologue", "ragged_fullres_rgb", "ragged_net_truth", "eval_sse", "range_audit",
        "splitk_epilogue", "nchw_to_nhwc", "nhwc_to_nchw", "split_to_nchw", "nchw_to_split"]
# the built-in caps of the launchers: this change keeps them exactly as they were
CAPS = {"head": 8192, "softmax_nchw": 8192, "dist313": 16384, "lab_post": 4096, "pcie_copy": 1024, "upsample_lab2rgb": 8192, "global_stats": 1024,
        "ingest_rgb": 4096, "fullres_rgb": 8192, "batch_prologue": 4096, "batch_fullres_rgb": 8192, "ragged_prologue": 4096,
        "ragged_fullres_rgb": 8192, "ragged_net_truth": 4096, "eval_sse": 256, "range_audit": 2048, "splitk_epilogue": 8192,
        "nchw_to_nhwc": 65535, "nhwc_to_nchw": 65535, "split_to_nchw": 65535, "nchw_to_split": 65535}
# launch sites that launch two template forms of their kernel from the one grid_blocks call
TWO_FORMS = {"nchw_to_nhwc", "head", "upsample_lab2rgb", "fullres_rgb", "range_audit", "splitk_epilogue"}


@pytest.fixture(scope="module")
def grid_selftest(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc (%s): tools/grid_selftest.cpp cannot be compiled" % HIPCC)
    out = str(tmp_path_factory.mktemp("grid_selftest"))
    subprocess.check_call(["make", "-C", CSRC, "grid_selftest", "BINDIR=" + out, "HIPCC=" + HIPCC], stdout=subprocess.DEVNULL)
    return os.path.join(out, "grid_selftest")


def test_clamp_hook_and_record(grid_selftest):
    run = subprocess.run([grid_selftest], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("grid_selftest: ok (21 tags)"), run.stdout + run.stderr


def _sources():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")))}


def _header_tags():
    text = open(os.path.join(CSRC, "idc_grid.h")).read()
    body = re.search(r"#define IDC_FOR_EACH_GRID_TAG\(X\)(.*?)\n\n", text, re.S).group(1)
    return re.findall(r"X\((\w+)\)", body)


def test_the_header_lists_the_21_tags_once():
    assert _header_tags() == TAGS
    text = open(os.path.join(CSRC, "idc_grid.h")).read()
    # plain C++: tools/grid_selftest.cpp includes it alone
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", text) == ["string.h"] and "__global__" not in text and "__device__" not in text


def test_every_tag_is_passed_to_grid_blocks_at_exactly_one_launch_site():
    calls = []          # (file, tag, built-in cap, the launcher's text from the call to its return)
    for name, text in _sources().items():
        for m in re.finditer(r"grid_blocks\(GridTag::(\w+),[^;]*?,\s*(\d+)\);", text):
            calls.append((name, m.group(1), int(m.group(2)), text[m.end():text.index("return hipGetLastError();", m.end())]))
        assert len(re.findall(r"\bgrid_blocks\(", text)) == len([c for c in calls if c[0] == name]), "%s: a grid_blocks call of another form" % name
    assert sorted(c[1] for c in calls) == sorted(TAGS), sorted(c[1] for c in calls)
    for name, tag, cap, body in calls:
        assert cap == CAPS[tag], "%s: built-in cap %d, was %d" % (tag, cap, CAPS[tag])
        launches = re.findall(r"hipLaunchKernelGGL\(\s*(\w+)(?:<[^>]*>)?,\s*dim3\(([^)]*)\)", body)
        assert len(launches) == (2 if tag in TWO_FORMS else 1), (tag, launches)
        assert len(set(k for k, _ in launches)) == 1, (tag, launches)                  # two launches: two template forms of ONE kernel
        for kernel, grid in launches:
            assert kernel == tag + "_kernel", (tag, kernel)
            assert re.fullmatch(r"blocks(, n)?", grid), "%s: launched on dim3(%s), not on the grid_blocks count" % (tag, grid)


def test_no_launcher_clamps_a_grid_of_its_own():
    for name, text in _sources().items():
        for line in text.splitlines():
            if "blocks" in line:
                assert not re.search(r"<\s*\d+\s*\?[^:;]*:\s*\d+", line), "%s clamps a grid outside grid_blocks: %s" % (name, line.strip())
                assert not re.search(r"if\s*\(\s*blocks\s*>\s*\d+\s*\)\s*blocks\s*=", line), "%s clamps a grid outside grid_blocks: %s" % (name, line.strip())


def test_option_and_entry_points_are_declared_and_wired():
    from interactive_deep_colorization_amd import _native as N
    from interactive_deep_colorization_amd import engine
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    assert '"grid_cap"' in header and "TEST HOOK" in header[header.index('"grid_cap"'):header.index('"grid_cap"') + 40]
    for sym in ("idc_grid_last", "idc_grid_tag"):
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in N.EXPORTED_SYMBOLS and hasattr(N.load(), sym), sym
    # no device is needed for either: the tags in the header's order, a record of zeros before any launch, statuses
    assert engine.grid_tags() == TAGS
    assert N.load().idc_grid_tag(-1) is None and N.load().idc_grid_tag(len(TAGS)) is None
    for t in TAGS:                                      # (0, 0) in a process that has launched nothing; blocks never above want
        want, blocks = engine.grid_last(t)
        assert 0 <= blocks <= max(want, 1) and (want > 0) == (blocks > 0), (t, want, blocks)
    with pytest.raises(N.IdcError) as ei:
        engine.grid_last("no_such_tag")
    assert ei.value.status == -1
    with pytest.raises(N.IdcError) as ei:
        engine.set_option("grid_cap", -1)
    assert ei.value.status == -1
    engine.set_option("grid_cap", 3)
    engine.set_option("grid_cap", 0)
