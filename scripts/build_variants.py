"""Variant builds of the library for A/B experiments (scripts/kbench.py --lib scripts/ab/<name>.so)."""
import sys
sys.path.insert(0, __file__.rsplit("/", 2)[0])
from pygenray_amd import _lib
VARIANTS = {"plain": [], "timing": ["-DPGR_TIMING"], "wavetimes": ["-DPGR_WAVE_TIMES"], "svctiming": ["-DPGR_SVC_TIMING"]}
# (the round-3 sample-store and service-timing switches -- PGR_SAMPLE_RING, PGR_WAVE_RING, PGR_DEFER_STORES,
# PGR_STORE_EXPERIMENT, PGR_DBG_REPLAY, PGR_DBG_SAMPLE_TRIPS -- left the kernel with
# scripts/experiments/r03_sample_store_experiments.patch; it applies to commit c081c9f (a worktree of that commit builds them again))
# (the rejected arithmetic and table-layout experiments -- pow2ulp, noreplay, libmtrig, nobandtab, pow2n, noziv, keepk0,
# pinlit, pinlit_nop, nopin_p, cellrec, rowpairs; PGR_POW_2ULP, PGR_NO_REPLAY, PGR_LIBM_TRIG, PGR_NO_BAND_TABLE,
# PGR_POW_TWO_NEWTON, PGR_STRICT, PGR_CELL_RECORDS, PGR_ROW_PAIRS and the -D overrides of PGR_KEEP_K / PGR_PIN_* -- left the
# sources after commit 22d856e, where this script still builds them)
for name in (sys.argv[1:] or VARIANTS):
    print(name, _lib.build(force=True, out=_lib.CSRC + f"/../../scripts/ab/{name}.so", extra_flags=VARIANTS[name], verbose=True), flush=True)
