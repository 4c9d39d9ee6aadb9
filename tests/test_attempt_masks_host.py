"""tests/attempt_masks_host.c -- the host twins of the mask helpers of a step attempt's tail (pgr_mask_lt_const,
pgr_mask_reached, pgr_factor_limit / pgr_step_factor, pgr_lane_pending: csrc/pgr_crmath.h) against the plain comparisons they
replace, on the doubles next to every threshold, zeros, infinities, NaNs of both signs, subnormals and 1e6 random operands
each -- built as a stand-alone program, once plainly and once with -fsanitize=address,undefined (that build skipped, with the
reason, where gcc has no sanitizer runtime), and run directly.  The kernel's own lines run on the GPU in
tests/test_attempt_decisions.py.  CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = ["gcc", "-O1", "-g", "-std=gnu99", "-ffp-contract=off", "-fno-fast-math", os.path.join(HERE, "attempt_masks_host.c"), "-lm"]


def _run(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = p.stdout + p.stderr
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-2000:]
    assert p.returncode == 0 and out.startswith("ok:"), out[-2000:]


def test_mask_predicates_equal_the_comparisons_they_replace(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc here")
    exe = str(tmp_path / "attempt_masks_host")
    subprocess.check_call(BASE + ["-o", exe])
    _run(exe)


def test_mask_predicates_under_the_sanitizers(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc here")
    has_runtime = all(os.path.isabs(subprocess.run(["gcc", f"-print-file-name={lib}"], capture_output=True, text=True).stdout.strip())
                      for lib in ("libasan.so", "libubsan.so"))
    if not has_runtime:
        pytest.skip("gcc has no sanitizer runtime here: the plain build above has run the same checks")
    exe = str(tmp_path / "attempt_masks_host_san")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    subprocess.check_call(BASE[:1] + san + BASE[1:] + ["-o", exe])
    _run(exe)
