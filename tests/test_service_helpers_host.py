"""tests/service_helpers_host.c -- the host twins of the mask helpers the bounce service's replay uses (pgr_sign_mask,
pgr_mask_select: csrc/pgr_crmath.h), the masked halvings and brentq iterations against the compare form -- built as a
stand-alone program with -fsanitize=address,undefined and run once (skipped, with the reason, where gcc has no sanitizer
runtime).  The program restates the kernel's halving and phase-2 iteration: it guards the two helpers and the algebra, not the
kernel's own lines, which tests/test_service_paths.py runs on the GPU.  CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_mask_selects_replay_the_compare_form_bit_for_bit(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc here")
    exe = str(tmp_path / "service_helpers_host")
    base = ["gcc", "-O1", "-g", "-std=gnu99", "-ffp-contract=off", "-fno-fast-math", os.path.join(HERE, "service_helpers_host.c"),
            "-lm", "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    has_runtime = all(os.path.isabs(subprocess.run(["gcc", f"-print-file-name={lib}"], capture_output=True, text=True).stdout.strip())
                      for lib in ("libasan.so", "libubsan.so"))
    if not has_runtime:
        pytest.skip("gcc has no sanitizer runtime here: the program is only meaningful as a sanitized build")
    subprocess.check_call(base[:1] + san + base[1:])     # (the sanitized build must succeed)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = p.stdout + p.stderr
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-2000:]
    assert p.returncode == 0 and out.startswith("ok:"), out[-2000:]
