"""The planner without a device: tools/plan_dump.cpp builds a configuration's graph, runs plan_forward and prints the layer table's name /
kernel / launches columns.  Held, string for string, against tests/golden/plan_tables.json: the tables HipColorizer.layer_table() gave on an
MI355X after one forward with idc_set_option("kwave_chain", 0) (the persistent trunk chain is decided at launch time, not planned), recorded from
the commit the file names -- the last one whose planner lived inside run_graph."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, REPO

CSRC = os.path.join(REPO, "interactive_deep_colorization_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAG_BITS = {"dist": 0x1, "global_hints": 0x4, "dist313": 0x8}

with open(os.path.join(GOLDEN, "plan_tables.json")) as _f:
    TABLES = json.load(_f)


def _id(cfg):
    opts = "".join(" %s=%d" % kv for kv in sorted(cfg["options"].items()))
    return "%dx%d %s (%d,%d)%s%s" % (cfg["H"], cfg["W"], cfg["precision"], cfg["max_batch"], cfg["n"], "".join(" " + f for f in cfg["flags"]), opts)


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc (%s): tools/plan_dump.cpp cannot be compiled" % HIPCC)
    assert os.path.exists(os.path.join(CSRC, "libideepcolor_hip.so")), "plan_dump links the built library: run __graft_entry__.build() first"
    out = str(tmp_path_factory.mktemp("plan_dump"))
    subprocess.check_call(["make", "-C", CSRC, "plan_dump", "BINDIR=" + out, "HIPCC=" + HIPCC], stdout=subprocess.DEVNULL)
    return os.path.join(out, "plan_dump")


@pytest.mark.parametrize("cfg", TABLES["configs"], ids=_id)
def test_plan_dump_matches_the_recorded_layer_table(plan_dump, cfg):
    flags = sum(FLAG_BITS[f] for f in cfg["flags"])
    cmd = [plan_dump, cfg["precision"], str(flags)] + [str(cfg[k]) for k in ("H", "W", "max_batch", "n")]
    cmd += ["%s=%d" % kv for kv in sorted(cfg["options"].items())]
    rows = [line.split("\t") for line in subprocess.check_output(cmd, text=True).splitlines()]
    want = [[name, kernel, str(launches)] for name, kernel, launches in cfg["rows"]]
    assert rows == want, "\n".join("%-16s %-40s | %s" % (w[0], w[1], r[1]) for w, r in zip(want, rows) if w != r)


def test_golden_covers_the_configurations_and_names_its_commit():
    assert len(TABLES["configs"]) == 17 and len(TABLES["recorded_from"]) >= 7
    assert {c["precision"] for c in TABLES["configs"]} == {"bf16", "fp32", "fp16x3", "bf16x6", "fp16"}
