"""The plan of a pipelined batch (csrc/idc_batch.h) without a device: tools/batch_selftest.cpp checks the hint clipping rule, every argument
check of plan_batch with its status and text (and that the earlier of two violations answers), the byte layout of the metadata block and the
pieces for same-size and ragged batches at n = 1 and n = max_batch, fill_batch_meta on a list that ends in dropped hints (a canary behind
meta_bytes, and an exactly-sized block for the sanitizer build), the ragged image table and the copy runs in both directions -- all against
literals written in the program.  Built and run plain and with SAN=1 (address + undefined-behaviour sanitizers on this host-only program)."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "interactive_deep_colorization_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module", params=["plain", "san"])
def batch_selftest(request, tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc (%s): tools/batch_selftest.cpp cannot be compiled" % HIPCC)
    out = str(tmp_path_factory.mktemp("batch_selftest_" + request.param))
    cmd = ["make", "-C", CSRC, "batch_selftest", "BINDIR=" + out, "HIPCC=" + HIPCC] + (["SAN=1"] if request.param == "san" else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return os.path.join(out, "batch_selftest")


def test_batch_plan_layouts_refusals_and_copy_runs(batch_selftest):
    run = subprocess.run([batch_selftest], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("batch_selftest: ok"), run.stdout + run.stderr
