"""The owners of csrc/idc_mem.h without a device: tools/mem_selftest.cpp instantiates them over counting fake allocators (a live set, an injected
k-th failure, an abort on a double or foreign release) and checks capacity, grow order, floors, failure-and-retry over a five-buffer sequence, moves,
reset and that nothing is left at exit.  Built here without a sanitizer (`make mem_selftest SAN=1` is the sanitizer build, for a CPU machine)."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "interactive_deep_colorization_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def mem_selftest(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc (%s): tools/mem_selftest.cpp cannot be compiled" % HIPCC)
    out = str(tmp_path_factory.mktemp("mem_selftest"))
    subprocess.check_call(["make", "-C", CSRC, "mem_selftest", "BINDIR=" + out, "HIPCC=" + HIPCC], stdout=subprocess.DEVNULL)
    return os.path.join(out, "mem_selftest")


def test_owners_release_exactly_once_and_retry_after_a_failed_allocation(mem_selftest):
    run = subprocess.run([mem_selftest], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("mem_selftest: ok"), run.stdout + run.stderr

