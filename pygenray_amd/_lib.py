"""ctypes binding of the C ABI in include/pgr.h (libpgr_hip.so).

The product path is HIP only: if the library is missing or cannot be loaded this module
raises -- there is no CPU fallback (the CPU oracle under oracle/ is test infrastructure and
is never imported from here).
"""
import ctypes
import os
import re
import sys
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
REFERENCE_LIB = os.path.join(CSRC, "libpgr_hip.so")
CONTRACTED_LIB = os.path.join(CSRC, "libpgr_hip_fma.so")
# fast-honor-pragmas: a*b + c fused everywhere EXCEPT where the source says `#pragma clang fp contract(off)` (grid_at,
# pgr_device.h: the np.linspace / table coordinates the histogram and the look-ups must reproduce bit for bit); a direct
# device compile with plain `fast` ignores the pragma (tests/test_host.py)
CONTRACTED_FLAGS = ["-DPGR_FMA", "-ffp-contract=fast-honor-pragmas"]


class PgrError(RuntimeError):
    pass


# Which arithmetic this PROCESS computes in -- an import-time choice, one library per process:
#   PGR_ARITH=reference (default)  libpgr_hip.so: the reference's IEEE operations in the reference's order, correctly
#                                  rounded div / sqrt / pow / asin / sin -- bit-identical to the CPU oracle; every parity
#                                  statement of this package is about THIS build;
#   PGR_ARITH=contracted           libpgr_hip_fma.so: the same sources with FMA contraction allowed (a*b + c fused, 2-ulp
#                                  reciprocal square root): ~10 % faster, statistically as close to pygenray as pygenray is
#                                  to itself (its numba kernels are fastmath=True, REF/integration_processes.py:26, and
#                                  SciPy's stage sums run through BLAS), but NOT the oracle's bits: no bit-parity claim.
ARITH = os.environ.get("PGR_ARITH", "reference").strip().lower() or "reference"
if ARITH not in ("reference", "contracted"):
    raise PgrError(f"PGR_ARITH={ARITH!r}: expected 'reference' (default) or 'contracted'")
LIB_PATH = CONTRACTED_LIB if ARITH == "contracted" else REFERENCE_LIB
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -disable-machine-licm: the bounce code's asin / sin / pow are inlined polynomials; machine LICM
# hoists their ~60 fp64 coefficients out of the WHOLE step loop into registers (235-256 VGPRs, 140-170
# SGPR spills); without it the kernel needs 147-162 VGPRs and 33-92 SGPR spills, and the step loop,
# whose own constants never fitted anyway, gets up to 3 % faster.  (Three waves per SIMD then fit,
# but measured slower: 1e6 rays 45.0 vs 42.4 ms, 180 000 rays 13.1 vs 9.8 ms -- a workgroup holds
# its CU until its last wave ends and the fans are VALU-bound already.)
# -ffp-contract=off: the reference's arithmetic (build_contracted() appends CONTRACTED_FLAGS, whose
# -ffp-contract=fast-honor-pragmas wins: contraction everywhere but inside `#pragma clang fp contract(off)`).
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-mllvm", "-disable-machine-licm",
               "-ffp-contract=off"]

RAY_STATUS = {0: "ok", 1: "vertical", 2: "bbox", 3: "backward", 4: "step_too_small",
              5: "max_steps", 6: "bottom_angle_range", 7: "event_error", 8: "skipped"}

# The C ABI is stated once, in include/pgr.h: its prototypes and PGR_* constants are read from there at import.
HEADER = os.path.join(_HERE, "..", "include", "pgr.h")
_BY_VALUE = {"double": ctypes.c_double, "int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
             "uint32_t": ctypes.c_uint32}
_RETURNS = {"int": ctypes.c_int, "void": None, "const char*": ctypes.c_char_p}


def parse_header(text):
    """The C ABI a header text declares -> (prototypes, constants): prototypes maps every function `pgr_*` to its ctypes
    (restype, argtypes), constants every `#define PGR_* <integer>[u]` to its value.  The five by-value types of the ABI map
    to their ctypes; a pointer, an array and a function-pointer typedef of the header are c_void_p (which takes an address,
    None, a ctypes pointer / array / callback or byref(...) as they are); any other by-value type is an error."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {n: int(v) for n, v in re.findall(r"^[ \t]*#define[ \t]+(PGR_\w+)[ \t]+(\d+)u?[ \t]*$", text, re.M)}
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{|\}', " ", text, flags=re.M)
    fn_typedefs = set(re.findall(r"\btypedef\b[^;]*?\(\s*\*\s*(\w+)\s*\)\s*\(", text))
    prototypes = {}
    for ret, name, params in re.findall(r"(?:^|;)\s*([\w\s*]+?)\s*\b(pgr_\w+)\s*\(([^()]*)\)\s*(?=;)", text):
        ret = re.sub(r"\s*\*\s*", "*", " ".join(ret.split()))
        if ret not in _RETURNS:
            raise PgrError(f"include/pgr.h: {name} returns {ret!r}, a type the binding does not know")
        argtypes = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            words = [w for w in p.split() if w != "const"]
            kind = " ".join(words[:-1] if len(words) > 1 else words)   # (the last word is the parameter's name)
            if "*" in p or "[" in p or kind in fn_typedefs:
                argtypes.append(ctypes.c_void_p)
            elif kind in _BY_VALUE:
                argtypes.append(_BY_VALUE[kind])
            else:
                raise PgrError(f"include/pgr.h: {name} takes `{' '.join(p.split())}` by value, a type the binding does "
                               "not know (add it to _BY_VALUE; it is not bound as a pointer by default)")
        prototypes[name] = (_RETURNS[ret], argtypes)
    return prototypes, constants


def _header_text(path):
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise PgrError(f"{path}: the C ABI header cannot be read ({e}); pygenray_amd binds libpgr_hip.so from it and runs "
                       "from its source tree") from None


def read_abi(header):
    """The C ABI `header` (include/pgr.h) states, itself and in every `#include "pgr_*.h"` of it, in order -> (paths,
    {file name: that header's own prototypes}, constants); a name two headers declare is an error."""
    bare = re.sub(r"/\*.*?\*/|//[^\n]*", " ", _header_text(header), flags=re.S)
    paths = [header] + [os.path.join(os.path.dirname(header), n)
                        for n in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"(pgr_\w+\.h)"', bare, re.M)]
    by_header, constants, owner = {}, {}, {}
    for path in paths:
        name = os.path.basename(path)
        by_header[name], consts = parse_header(_header_text(path))
        constants.update(consts)
        for fn in by_header[name]:
            if owner.setdefault(fn, name) != name:
                raise PgrError(f"{fn} is declared in {owner[fn]} and again in {name}")
    return paths, by_header, constants


# (pgr.h first, then the products that came with a header of their own, DESIGN.md sections 16-24; PROTOTYPES: what load() binds)
HEADERS, HEADER_PROTOTYPES, _CONSTANTS = read_abi(HEADER)
PROTOTYPES = {fn: proto for protos in HEADER_PROTOTYPES.values() for fn, proto in protos.items()}
globals().update(_CONSTANTS)   # PGR_TERMINATE_BACKWARDS, PGR_SAMPLE_MAJOR, ... PGR_OPT_D2H_REGISTER

_REBUILD = "`python -c 'import __graft_entry__ as g; g.build()'`"
_lib = None


def _llvm_bin():
    return os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "lib", "llvm", "bin")


def _relayout(td, verbose):
    """Second pass of the build (pygenray_amd/_isa_layout.py): re-encode 4-byte VALU instructions as
    8-byte ones where that keeps 8-byte instructions from straddling a 32-byte fetch window, then
    assemble, link and bundle the device code again and put it into the host object.  Works on the
    intermediates hipcc -save-temps left in `td`; returns the path of the finished library."""
    import re
    from . import _isa_layout
    B = _llvm_bin()
    dev_s = os.path.join(td, "pgr_hip-hip-amdgcn-amd-amdhsa-gfx950.s")
    dev_o = os.path.join(td, "pgr_hip-hip-amdgcn-amd-amdhsa-gfx950.o")
    host_s = os.path.join(td, "pgr_hip-host-x86_64-unknown-linux-gnu.s")
    layout = _isa_layout.object_layout(os.path.join(B, "llvm-objdump"), dev_o)
    with open(dev_s) as f:
        text, report = _isa_layout.relayout(f.read(), layout)
    dev2_s, dev2_o = os.path.join(td, "dev2.s"), os.path.join(td, "dev2.o")
    dev2_out, fb = os.path.join(td, "dev2.out"), os.path.join(td, "dev2.hipfb")
    with open(dev2_s, "w") as f:
        f.write(text)
    run = lambda c: subprocess.check_call(c, cwd=td)
    run([os.path.join(B, "clang"), "-cc1as", "-triple", "amdgcn-amd-amdhsa", "-filetype", "obj",
         "-main-file-name", "pgr_hip.hip", "-target-cpu", "gfx950", "-mrelocation-model", "pic",
         "-o", dev2_o, dev2_s])
    # the re-encoded object must hold the same instructions in the same order
    after = _isa_layout.object_layout(os.path.join(B, "llvm-objdump"), dev2_o)
    _isa_layout.check_same_program(layout, after)
    run([os.path.join(B, "lld"), "-flavor", "gnu", "-m", "elf64_amdgpu", "--no-undefined", "-shared",
         "-plugin-opt=-amdgpu-internalize-symbols", "-plugin-opt=mcpu=gfx950", "-plugin-opt=O3",
         "--whole-archive", "-o", dev2_out, dev2_o, "--no-whole-archive"])
    run([os.path.join(B, "clang-offload-bundler"), "-type=o", "-bundle-align=4096",
         "-targets=host-x86_64-unknown-linux-gnu,hipv4-amdgcn-amd-amdhsa--gfx950",
         "-input=/dev/null", f"-input={dev2_out}", f"-output={fb}"])
    # the host assembly carries the fat binary as one string: point it at the new bundle instead
    with open(host_s, "rb") as f:
        h = f.read()
    i = h.index(b'\t.asciz\t"__CLANG_OFFLOAD_BUNDLE__')
    j = h.index(b"\n", i)
    k = h.index(b"\n", j + 1)
    m = re.match(rb"\t\.size\t(\S+), (\d+)", h[j + 1:k])
    if not m:
        raise RuntimeError("unexpected layout of the fat binary in the host assembly")
    h = (h[:i] + b'\t.incbin\t"' + fb.encode() + b'"\n\t.size\t' + m.group(1) + b", " +
         str(os.path.getsize(fb)).encode() + h[k:])
    # ... and say so in the library: pgr_build_info() reads this tag (same length, so nothing moves)
    b = sum(v[0] for v in report.values()); a = sum(v[1] for v in report.values())
    tag0 = b"PGR_BUILD_TAG:plain hipcc"
    k0 = h.index(tag0)
    k1 = h.index(b'"', k0)
    tag = (f"PGR_BUILD_TAG:relaid, {b} -> {a} straddling 8-byte instructions").encode()
    if len(tag) > k1 - k0:
        raise RuntimeError("build tag too long")
    h = h[:k0] + tag + b" " * (k1 - k0 - len(tag)) + h[k1:]
    host2_s, host2_o = os.path.join(td, "host2.s"), os.path.join(td, "host2.o")
    with open(host2_s, "wb") as f:
        f.write(h)
    run([os.path.join(B, "clang"), "-c", host2_s, "-o", host2_o])
    out = os.path.join(td, "relaid.so")
    run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, host2_o])
    if verbose:
        print(f"instruction layout: {b} -> {a} 8-byte instructions straddle a 32-byte fetch window "
              f"({sum(v[2] for v in report.values())} re-encoded as e64)")
    return out


def build_dependencies():
    """The files a library build reads: the one translation unit csrc/pgr_hip.hip, which includes every csrc/*.h (device
    building blocks, the fan kernel, the host side in pieces), the ABI headers, and the instruction-layout pass."""
    return [os.path.join(CSRC, "pgr_hip.hip")] + HEADERS + [os.path.join(_HERE, "_isa_layout.py")] + sorted(
        os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".h"))


def build(force=False, verbose=False, out=None, extra_flags=()):
    """Compile csrc/pgr_hip.hip (ONE translation unit; it includes every csrc/*.h) for gfx950 (cross-compiles without a GPU): hipcc, then the
    instruction-layout pass over its assembly (_relayout; PGR_NO_RELAYOUT=1 or any failure of that
    pass leaves the plain hipcc build in place).  The default builds the product, REFERENCE_LIB, whatever PGR_ARITH
    says; `out` / `extra_flags`: build a variant library somewhere else (build_contracted(), scripts/build_variants.py)."""
    import shutil
    import tempfile
    if extra_flags and out is None:
        raise ValueError("build(extra_flags=...) needs `out`: only the product's own recipe writes the product library")
    LIB_PATH = out or REFERENCE_LIB
    src = os.path.join(CSRC, "pgr_hip.hip")
    if not force and os.path.exists(LIB_PATH):
        if os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(d) for d in build_dependencies()):
            return LIB_PATH
    tmp = f"{LIB_PATH}.{os.getpid()}.tmp"   # never leave a half-written library behind
    td = tempfile.mkdtemp(prefix="pgr_build_")
    try:
        plain = os.path.join(td, "plain.so")
        cmd = [HIPCC] + HIPCC_FLAGS + list(extra_flags) + ["-save-temps", "-o", plain, src]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd, cwd=td)
        result = plain
        if not os.environ.get("PGR_NO_RELAYOUT"):
            try:
                result = _relayout(td, verbose)
            except Exception as e:  # the plain build is complete and correct: keep it, say why
                print(f"pygenray_amd: instruction-layout pass skipped ({type(e).__name__}: {e})", file=sys.stderr)
        shutil.copyfile(result, tmp)
        os.chmod(tmp, 0o755)
        os.replace(tmp, LIB_PATH)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
        shutil.rmtree(td, ignore_errors=True)
    return LIB_PATH


def build_contracted(force=False, verbose=False):
    """The PGR_ARITH=contracted library (libpgr_hip_fma.so) beside the product: same sources, FMA contraction allowed."""
    return build(force=force, verbose=verbose, out=CONTRACTED_LIB, extra_flags=CONTRACTED_FLAGS)


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).  Two
    HIP runtimes in one process do not work (the second one finds no GPUs, and a torch stream
    handed to the other runtime is undefined behaviour), so when torch is installed its copy is
    loaded first and libpgr_hip.so's DT_NEEDED libamdhip64.so.7 resolves to it -- whichever of
    torch / pygenray_amd is imported first.  Without torch the system runtime is used."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is not None and spec.origin:
            p = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            if os.path.exists(p):
                ctypes.CDLL(p, mode=ctypes.RTLD_GLOBAL)
    except Exception:
        pass


def load():
    """Load libpgr_hip.so and bind every prototype of include/pgr.h; raise loudly if it is absent (no fallback) or lacks one."""
    global _lib
    if _lib is not None:
        return _lib
    _preload_torch_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise PgrError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run {_REBUILD} (needs hipcc"
            + ("; PGR_ARITH=contracted loads the FMA-contracted variant, built by the same call or by "
               "pygenray_amd._lib.build_contracted()" if ARITH == "contracted" else "") +
            "). pygenray_amd has no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            header = next(h for h, protos in HEADER_PROTOTYPES.items() if name in protos)
            raise PgrError(f"{LIB_PATH} does not export {name}, which include/{header} declares: the library is older than "
                           f"the header. Rebuild it: {_REBUILD}.") from None
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise PgrError(load().pgr_last_error().decode())


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _addr(a):
    """The address of a NumPy buffer (None: NULL), as a c_void_p parameter takes it."""
    return None if a is None else a.ctypes.data


def _profile(nodes, values, what):
    """two host sequences, the first or None -> (nodes or None, values) float64, of equal length (`what` words the error)"""
    v = _c(values).reshape(-1)
    x = None if nodes is None else _c(nodes).reshape(-1)
    if x is not None and len(x) != len(v):
        raise ValueError(f"{what} must have equal length")
    return x, v


class _Fan:
    """The fan products on raw device pointers (ints), each stated once for both kinds of fan (`_entry` names a kind's entries,
    `_fan` holds their leading arguments): FanHandle, a device-resident fan, calls pgr_fan_<product>(handle, ...); _Buffers,
    caller buffers behind a <product>_device function, calls pgr_<product>_device(env, rows, n_rays, n_samples, x, ...), which
    takes the same arguments after those (include/pgr.h).  The docstrings speak of a FanHandle: S save ranges, M surviving rays."""

    def _call(self, product, *args, suffix=""):
        check(getattr(load(), self._entry % product + suffix)(*self._fan, *args))

    def _twin(self, product, weights, p0_ptr, *rest):
        """Tube entry `product` or, with `weights` (a device pointer, not 0 / None), its weighted twin `product`_w, whose one
        more argument follows p0 (include/pgr.h)."""
        if weights:
            return self._call(product, p0_ptr, weights, *rest, suffix="_w")
        self._call(product, p0_ptr, *rest)

    def boundary_loss(self, tables, out_ptr, nb_ptr=0, ns_ptr=0, stream=0):
        """pgr_fan_boundary_loss: out[S][M] (device pointer) = the boundary loss in dB of this fan's surviving rays up to
        every save range; `tables` = boundary_tables(...) (host); nb / ns [S][M] int32 device pointers or 0."""
        self._call("boundary_loss", *_table_args(tables), out_ptr, nb_ptr, ns_ptr, stream)

    def intensity(self, p0_ptr, depths_ptr, n_depths, out_ptr, stream=0, weights=0):
        """pgr_fan_intensity on raw device pointers (ints): out[n_depths][S] = the ray-tube intensity of this fan's surviving
        rays at the receiver depths (include/pgr.h); p0 holds the M surviving rays' launch slowness.  Enqueued on `stream`.
        `weights` (here and in beam_intensity / arrivals): a device pointer to [S][M] weights of g, which selects the entry's
        weighted twin (pgr_fan_intensity_w); 0: the unweighted entry."""
        self._twin("intensity", weights, p0_ptr, depths_ptr, int(n_depths), out_ptr, stream)

    def path_integral(self, a_depths, alpha, out_ptr, stream=0):
        """pgr_fan_path_integral: out[S][M] (device pointer) = the running path integral of this fan's surviving rays for
        the absorption profile alpha (dB/m) on the depth nodes a_depths (host sequences; a_depths None with one alpha)."""
        ad, al = _profile(a_depths, alpha, "a_depths and alpha")
        self._call("path_integral", _addr(ad), _addr(al), len(al), out_ptr, stream)

    def beam_intensity(self, p0_ptr, bottom_ptr, depths_ptr, n_depths, min_width, out_ptr, stream=0, weights=0):
        """pgr_fan_beam_intensity on raw device pointers (ints): out[n_depths][S] = the Gaussian-beam intensity of this fan's
        surviving rays at the receiver depths, bottom[S] the bottom depth at each save range (include/pgr.h)."""
        self._twin("beam_intensity", weights, p0_ptr, bottom_ptr, depths_ptr, int(n_depths), float(min_width), out_ptr, stream)

    def arrival_counts(self, p0_ptr, depths_ptr, n_depths, cols, counts_ptr, stream=0):
        """pgr_fan_arrival_counts: counts[n_depths][len(cols)] (int64, device pointer) = the arrivals of this fan's surviving
        rays at each receiver depth and requested column; `cols` is a host sequence of column indices (include/pgr.h)."""
        c = np.ascontiguousarray(cols, dtype=np.int32)
        self._call("arrival_counts", p0_ptr, depths_ptr, int(n_depths), _addr(c), len(c), counts_ptr, stream)

    def arrivals(self, p0_ptr, depths_ptr, n_depths, cols, offsets_ptr, n_arrivals, tube_ptr, w_ptr, t_ptr, p_ptr, i_ptr,
                 stream=0, weights=0):
        """pgr_fan_arrivals: the arrivals themselves, written from offsets[j * len(cols) + c] into tube (int32) / w / T / p /
        I (device pointers holding n_arrivals each)."""
        c = np.ascontiguousarray(cols, dtype=np.int32)
        self._twin("arrivals", weights, p0_ptr, depths_ptr, int(n_depths), _addr(c), len(c), offsets_ptr, int(n_arrivals),
                   tube_ptr, w_ptr, t_ptr, p_ptr, i_ptr, stream)

    def travel_time_kernel(self, ranges_ptr, n_ranges, depths_ptr, n_depths, column, out_ptr, stream=0):
        """pgr_fan_travel_time_kernel on raw device pointers (ints): out[M][n_ranges][n_depths] = the travel-time sensitivity
        kernel of this fan's surviving rays at save column `column` on the grid ranges x depths (include/pgr.h)."""
        self._call("travel_time_kernel", ranges_ptr, int(n_ranges), depths_ptr, int(n_depths), int(column), out_ptr, stream)

    def time_front(self, cols, t_ptr, z_ptr, p_ptr, turns_ptr, stream=0):
        """pgr_fan_time_front on raw device pointers (ints; 0 / None: not wanted): t / z / p [len(cols)][M] float64 = the
        surviving rays' samples at the save columns `cols` (a host sequence of column indices), turns [len(cols)][M] int32
        = their turning-point counts up to those columns (include/pgr.h).  Enqueued on `stream`."""
        c = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32)
        self._call("time_front", _addr(c), 0 if c is None else len(c), t_ptr, z_ptr, p_ptr, turns_ptr, stream)

    def caustic_index(self, nb_ptr, ns_ptr, kappa_ptr, stream=0):
        """pgr_fan_caustic_index on raw device pointers (ints): kappa[S][M] int32 = the caustics every tube of this fan's
        surviving rays has passed up to every save range; nb / ns [S][M] int32, the per-sample bounce counts boundary_loss
        writes, or 0 (a fan without bounces).  Enqueued on `stream`."""
        self._call("caustic_index", nb_ptr or None, ns_ptr or None, kappa_ptr, stream)

    def pressure(self, p0_ptr, q_ptr, frequency, depths_ptr, n_depths, re_ptr, im_ptr, stream=0, weights=0):
        """pgr_fan_pressure_w on raw device pointers (ints): re / im [n_depths][S] = the coherent sum of this fan's ray tubes
        at the receiver depths; q [S][M] int32 the tubes' phase index in quarter cycles or 0, `weights` as in ``intensity``
        or 0 (include/pgr.h)."""
        self._call("pressure", p0_ptr, weights or None, q_ptr or None, float(frequency), depths_ptr, int(n_depths), re_ptr, im_ptr,
                   stream, suffix="_w")

    def pressure_phi(self, p0_ptr, q_ptr, phi_ptr, frequency, depths_ptr, n_depths, re_ptr, im_ptr, stream=0, weights=0):
        """pgr_fan_pressure_phi on raw device pointers (ints): ``pressure`` with phi [S][M] float64, the lag in cycles every
        surviving ray has collected up to every save range (include/pgr_reflection.h); phi 0 is refused."""
        self._call("pressure", p0_ptr, weights or None, q_ptr or None, phi_ptr or None, float(frequency), depths_ptr,
                   int(n_depths), re_ptr, im_ptr, stream, suffix="_phi")

    def beam_pressure(self, p0_ptr, q_ptr, frequency, bottom_ptr, depths_ptr, n_depths, min_width, curvature, re_ptr, im_ptr,
                      stream=0, weights=0):
        """pgr_fan_beam_pressure_w on raw device pointers (ints): re / im [n_depths][S] = the coherent sum of this fan's
        Gaussian beams at the receiver depths; q and `weights` as in ``pressure``, bottom and min_width as in
        ``beam_intensity``, `curvature` false for the plain geometric beam (include/pgr_beam_coherent.h)."""
        self._call("beam_pressure", p0_ptr, weights or None, q_ptr or None, float(frequency), bottom_ptr, depths_ptr,
                   int(n_depths), float(min_width), int(bool(curvature)), re_ptr, im_ptr, stream, suffix="_w")

    def beam_arrival_counts(self, p0_ptr, q_ptr, bottom_ptr, depths_ptr, n_depths, min_width, cols, counts_ptr, stream=0,
                            weights=0):
        """pgr_fan_beam_arrival_counts_w on raw device pointers (ints): counts[n_depths][len(cols)] (int64) = the terms
        ``beam_pressure`` adds at each receiver depth and requested column; `cols` a host sequence of column indices, the
        other arguments ``beam_pressure``'s (include/pgr_beam_arrivals.h)."""
        c = np.ascontiguousarray(cols, dtype=np.int32)
        self._call("beam_arrival_counts", p0_ptr, weights or None, q_ptr or None, bottom_ptr, depths_ptr, int(n_depths),
                   float(min_width), _addr(c), len(c), counts_ptr, stream, suffix="_w")

    def beam_arrivals(self, p0_ptr, q_ptr, bottom_ptr, depths_ptr, n_depths, min_width, cols, curvature, offsets_ptr, n_arrivals,
                      tube_ptr, image_ptr, time_ptr, amp_ptr, qa_ptr, stream=0, weights=0):
        """pgr_fan_beam_arrivals_w: those terms themselves, written from offsets[j * len(cols) + c] into tube, image, qa
        (int32) and time, amplitude (float64), device pointers holding n_arrivals each."""
        c = np.ascontiguousarray(cols, dtype=np.int32)
        self._call("beam_arrivals", p0_ptr, weights or None, q_ptr or None, bottom_ptr, depths_ptr, int(n_depths),
                   float(min_width), _addr(c), len(c), int(bool(curvature)), offsets_ptr, int(n_arrivals), tube_ptr, image_ptr,
                   time_ptr, amp_ptr, qa_ptr, stream, suffix="_w")


class _Buffers(_Fan):
    """caller buffers as a fan: `fan` are the leading arguments of the one buffer entry the <product>_device function calls"""
    _entry = "pgr_%s_device"

    def __init__(self, *fan):
        self._fan = fan


def _buffers(env, n_rays, n_samples, x_ptr, *rows):
    """_Buffers of the rows of T / z / p [n_samples][n_rays] an entry reads on the save ranges x of the frame of `env`"""
    return _Buffers(env._h, *rows, int(n_rays), int(n_samples), x_ptr)


class EnvHandle:
    """Owns one pgr_env (environment tables resident in HBM on `device`)."""

    def __init__(self, cin, cpin, rin, zin, depths, depth_ranges, bottom_angles, device=0):
        L = load()
        cin, cpin, rin, zin = _c(cin), _c(cpin), _c(rin), _c(zin)
        depths, depth_ranges, bottom_angles = _c(depths), _c(depth_ranges), _c(bottom_angles)
        if cin.ndim != 2 or cin.shape != cpin.shape or cin.shape != (len(rin), len(zin)):
            raise ValueError("cin/cpin must have shape (len(rin), len(zin))")
        if not (len(depths) == len(depth_ranges) == len(bottom_angles)):
            raise ValueError("depths, depth_ranges and bottom_angles must have equal length")
        h = ctypes.c_void_p()
        check(L.pgr_env_create(ctypes.byref(h), int(device), _addr(cin), _addr(cpin), _addr(rin), _addr(zin),
                               len(rin), len(zin), _addr(depths), _addr(depth_ranges), _addr(bottom_angles),
                               len(depths)))
        self._h = h
        self.device = int(device)
        self.shape = cin.shape

    def query(self, what):
        return load().pgr_env_query(self._h, int(what))

    # tuning options of this environment (include/pgr.h; results never depend on them)
    _OPTIONS = {n[len("PGR_OPT_"):].lower(): v for n, v in _CONSTANTS.items() if n.startswith("PGR_OPT_")}

    def set_option(self, name, a, b=0):
        check(load().pgr_env_set_option(self._h, self._OPTIONS[name], int(a), int(b)))

    @property
    def range_independent(self):
        return bool(self.query(0))

    @property
    def lds_path(self):
        return bool(self.query(3))

    @property
    def blocked_layout(self):
        """True when a sample-major trajectory fan of this environment is best written sample-blocked ([ceil(S/4)][N][4],
        PGR_SAMPLE_BLOCKED): its tables stay in HBM / L2 and the LDS has room for the staging (include/pgr.h)."""
        return bool(self.query(8))

    def close(self):
        if getattr(self, "_h", None):
            load().pgr_env_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host-pointer entry (NumPy in / NumPy out) ----
    def shoot_fan(self, y0, source_range, receiver_range, num_range_save, rtol=1e-9, atol=1e-6,
                  terminate_backwards=True, max_steps=1_000_000, save=True, sample_major=False,
                  exact_bisection=False, exact_samples=False, stored_sign=False, compact=False, buffers=None):
        """``buffers``: (T, Z, P) float64 arrays of the right shape to write into (caller-owned, e.g.
        reused across fans) instead of fresh ones."""
        L = load()
        y0 = _c(y0).reshape(-1, 3)
        N, S = len(y0), int(num_range_save)
        r = np.linspace(source_range, receiver_range, S)
        flags = (PGR_TERMINATE_BACKWARDS if terminate_backwards else 0) | \
            (PGR_SAMPLE_MAJOR if sample_major else 0) | (PGR_EXACT_BISECTION if exact_bisection else 0) | \
            (PGR_EXACT_SAMPLES if exact_samples else 0) | (PGR_STORED_SIGN if stored_sign else 0) | \
            (PGR_COMPACT if (compact and sample_major) else 0)
        if save:
            shape = (S, N) if sample_major else (N, S)
            if buffers is not None:
                T, Z, P = buffers
                for b_ in (T, Z, P):
                    if b_.shape != shape or b_.dtype != np.float64 or not b_.flags.c_contiguous:
                        raise ValueError(f"buffers must be C-contiguous float64 arrays of shape {shape}")
            else:
                T = np.empty(shape); Z = np.empty(shape); P = np.empty(shape)
        else:
            T = Z = P = None
        end = np.empty((N, 3))
        nb = np.zeros(N, np.int32); ns = np.zeros(N, np.int32); st = np.zeros(N, np.int32)
        nsteps = np.zeros(N, np.int32); nrej = np.zeros(N, np.int32)
        check(L.pgr_shoot_fan(self._h, _addr(y0), N, float(source_range), float(receiver_range),
                              _addr(r), S, float(rtol), float(atol), flags, int(max_steps),
                              _addr(T), _addr(Z), _addr(P), _addr(end), _addr(nb), _addr(ns),
                              _addr(st), _addr(nsteps), _addr(nrej)))
        if save and compact and sample_major:
            # PGR_COMPACT: the trajectories of the M rays with status 0 sit as [S][M] at the start
            # of the buffers
            M = int(np.count_nonzero(st == 0))
            if M < N:
                T, Z, P = (a.reshape(-1)[:S * M].reshape(S, M) for a in (T, Z, P))
        return dict(r=r, T=T, z=Z, p=P, end=end, n_bott=nb, n_surf=ns, status=st, n_steps=nsteps,
                    n_rej=nrej)

    # ---- device-pointer entry (integers are raw device addresses, e.g. tensor.data_ptr()) ----
    def shoot_fan_device(self, y0_ptr, N, source_range, receiver_range, r_ptr, S, rtol, atol, flags,
                         max_steps, T_ptr, Z_ptr, P_ptr, end_ptr, nb_ptr, ns_ptr, st_ptr,
                         nsteps_ptr, nrej_ptr, stream=0):
        check(load().pgr_shoot_fan_device(self._h, y0_ptr, int(N), float(source_range), float(receiver_range), r_ptr, int(S),
                                          float(rtol), float(atol), int(flags), int(max_steps), T_ptr, Z_ptr, P_ptr, end_ptr,
                                          nb_ptr, ns_ptr, st_ptr, nsteps_ptr, nrej_ptr, stream))

    def debug_step(self, t, y, h, rtol=1e-9, atol=1e-6):
        """One RK45 step attempt per (t, y, h): y_new[3], f_new[3], error_norm, 0.9 err**-0.2, f[3]."""
        t = _c(t); y = _c(y).reshape(-1, 3); h = _c(h)
        out = np.empty((len(t), 11))
        check(load().pgr_debug_step(self._h, _addr(t), _addr(y), _addr(h), len(t), float(rtol), float(atol), _addr(out)))
        return out

    def eigen_refine(self, th1, th2, z1, z2, receiver_depth, source_depth, source_range, receiver_range, c_source,
                     rtol=1e-9, atol=1e-6, terminate_backwards=True, max_steps=1_000_000, ztol=1.0, max_iter=20,
                     slowness=None):
        """pgr_eigen_refine_depths_fn: the false-position loop of REF/eigenrays.py:206-268 for all brackets, on the device.
        `receiver_depth`: one depth for all brackets, or one per bracket (the brackets of several receiver depths
        searched together).  `slowness(ode_angles_deg) -> p0`: the caller's sin(radians(.)) / c for the trial rays (the shim
        passes NumPy's, the reference's arithmetic); None: the device's correctly rounded sine.  The callback runs inside
        the search with this environment's workspace lock held: it must not shoot rays or search on THIS EnvHandle
        (include/pgr.h); plain NumPy arithmetic, as the shim's, is what it is for."""
        th1, th2, z1, z2 = (_c(a).reshape(-1) for a in (th1, th2, z1, z2))
        n = len(th1)
        rd = _c(np.broadcast_to(np.asarray(receiver_depth, dtype=float), (n,)))
        theta = np.full(n, np.nan); zend = np.full(n, np.nan); tend = np.full(n, np.nan)
        state = np.zeros(n, np.int32); ntrial = np.zeros(n, np.int32)
        launches = ctypes.c_int32(0)
        dp = ctypes.POINTER(ctypes.c_double)
        FN = ctypes.CFUNCTYPE(None, dp, ctypes.c_int64, dp, ctypes.c_void_p)   # pgr_slowness_fn
        failure = []

        def _cb(ang_p, m, out_p, _user):
            try:    # (an exception must not unwind through the C frames: it is re-raised when the call has returned)
                ang = np.ctypeslib.as_array(ang_p, shape=(m,))
                np.ctypeslib.as_array(out_p, shape=(m,))[:] = slowness(ang)
            except BaseException as exc:   # noqa: BLE001
                failure.append(exc)
                np.ctypeslib.as_array(out_p, shape=(m,))[:] = np.nan
        cb = FN(_cb) if slowness is not None else None   # (alive until the call has returned)
        check(load().pgr_eigen_refine_depths_fn(
            self._h, n, _addr(th1), _addr(th2), _addr(z1), _addr(z2), _addr(rd), float(source_depth), float(source_range),
            float(receiver_range), float(c_source), float(rtol), float(atol),
            PGR_TERMINATE_BACKWARDS if terminate_backwards else 0, int(max_steps), float(ztol), int(max_iter), _addr(theta),
            _addr(state), _addr(ntrial), _addr(zend), _addr(tend), ctypes.byref(launches), cb, None))
        if failure:
            raise failure[0]
        return dict(theta=theta, state=state, n_trial=ntrial, z_end=zend, t_end=tend, launches=int(launches.value))

    def last_instance(self):
        """pgr_debug_last_instance: dict(lds_tab, zm, save, persist, blocks, threads, lds_bytes, queue_tail) of the last fan launch."""
        out = (ctypes.c_int32 * 8)()
        check(load().pgr_debug_last_instance(self._h, out))
        return dict(zip(("lds_tab", "zm", "save", "persist", "blocks", "threads", "lds_bytes", "queue_tail"), (int(v) for v in out)))

    def last_instance_log(self):
        """pgr_debug_last_instance_log: 1 when the last fan launch selected an instance that writes a bounce log, 0 when not,
        -1 before any launch."""
        return int(load().pgr_debug_last_instance_log(self._h))

    def eval_points(self, x, y):
        x = _c(x); y = _c(y).reshape(-1, 3)
        out = np.empty((len(x), 10))
        check(load().pgr_eval_points(self._h, _addr(x), _addr(y), len(x), _addr(out)))
        return out


class FanHandle(_Fan):
    """A fan whose results stay in HBM (pgr_fan_*, include/pgr.h): launched in the constructor (returns while the
    kernel runs), per-ray arrays and trajectories fetched on demand, the products of _Fan computed where it is."""
    _entry = "pgr_fan_%s"
    _fan = property(lambda self: (self._h,))

    def __init__(self, env, x0, x1, S, y0=None, ode_angles_deg=None, source_depth=0.0, c_source=1.0, rtol=1e-9,
                 atol=1e-6, terminate_backwards=True, max_steps=1_000_000, stored_sign=False, exact_samples=False,
                 exact_bisection=False, p0=None, skip_nan=False, max_bounces=None):
        """``max_bounces`` (an int >= 1; None: no log, pgr_fan_launch as ever): pgr_fan_launch_log -- the fan keeps a bounce
        log of that many slots per ray (``fetch_bounces``, ``boundary_loss``)."""
        L = load()
        self._env = env   # keeps the environment (its stream, its tables) alive
        if y0 is not None:
            y0 = _c(y0).reshape(-1, 3)
            n = len(y0)
        elif p0 is not None:      # the caller's own sin(radians(angle)) / c per ray (PGR_LAUNCH_SLOWNESS)
            ode_angles_deg = _c(p0).reshape(-1)
            n = len(ode_angles_deg)
        else:
            ode_angles_deg = _c(ode_angles_deg).reshape(-1)
            n = len(ode_angles_deg)
        self.N, self.S = n, int(S)
        flags = (PGR_TERMINATE_BACKWARDS if terminate_backwards else 0) | (PGR_STORED_SIGN if stored_sign else 0) | \
            (PGR_EXACT_SAMPLES if exact_samples else 0) | (PGR_EXACT_BISECTION if exact_bisection else 0) | \
            (PGR_LAUNCH_SLOWNESS if p0 is not None else 0) | (PGR_SKIP_NAN_Y0 if skip_nan else 0)
        h = ctypes.c_void_p()
        self.K = 0 if max_bounces is None else int(max_bounces)
        if max_bounces is None:
            check(L.pgr_fan_launch(env._h, _addr(y0), _addr(ode_angles_deg), float(source_depth), float(c_source), n,
                                   float(x0), float(x1), self.S, float(rtol), float(atol), flags, int(max_steps),
                                   ctypes.byref(h)))
        else:
            check(L.pgr_fan_launch_log(env._h, _addr(y0), _addr(ode_angles_deg), float(source_depth), float(c_source), n,
                                       float(x0), float(x1), self.S, float(rtol), float(atol), flags, int(max_steps),
                                       self.K, ctypes.byref(h)))
        self._h = h
        self.M = None

    def fetch_bounces(self):
        """pgr_fan_fetch_bounces: the bounce log of the surviving rays -> x, p (K, M) float64 and kind (K, M) int8; slots
        never written hold NaN, NaN, -1."""
        if self.M is None:
            self.wait()
        x, p = np.empty((self.K, self.M)), np.empty((self.K, self.M))
        k = np.empty((self.K, self.M), np.int8)
        check(load().pgr_fan_fetch_bounces(self._h, _addr(x), _addr(p), _addr(k)))
        return x, p, k

    def wait(self):
        n, m = ctypes.c_int64(0), ctypes.c_int64(0)
        check(load().pgr_fan_wait(self._h, ctypes.byref(n), ctypes.byref(m)))
        self.M = int(m.value)
        return int(n.value), self.M

    def fetch_rays(self):
        n = self.N
        end = np.empty((n, 3))
        nb = np.empty(n, np.int32); ns = np.empty(n, np.int32); st = np.empty(n, np.int32)
        n1 = np.empty(n, np.int32); n2 = np.empty(n, np.int32)
        check(load().pgr_fan_fetch_rays(self._h, _addr(end), _addr(nb), _addr(ns), _addr(st), _addr(n1), _addr(n2)))
        self.M = int(np.count_nonzero(st == 0))
        return dict(end=end, n_bott=nb, n_surf=ns, status=st, n_steps=n1, n_rej=n2)

    def fetch_rays_compact(self, per_ray=None):
        """The surviving rays only (launch order): end [M, 3], n_bott / n_surf [M] int64 and, squeezed the same way,
        the caller's per-ray array `per_ray` [N] -> [M]."""
        if self.M is None:
            self.wait()
        m = self.M
        end = np.empty((m, 3)); nb = np.empty(m, np.int64); ns = np.empty(m, np.int64)
        src = None if per_ray is None else _c(per_ray).reshape(-1)
        out = None if per_ray is None else np.empty(m)
        check(load().pgr_fan_fetch_rays_compact(self._h, _addr(src), _addr(out), _addr(end), _addr(nb), _addr(ns)))
        return dict(end=end, n_bott=nb, n_surf=ns, per_ray=out)

    def status(self):
        """status [N] (waits for the kernel)."""
        st = np.empty(self.N, np.int32)
        check(load().pgr_fan_fetch_rays(self._h, None, None, None, _addr(st), None, None))
        self.M = int(np.count_nonzero(st == 0))
        return st

    def fetch_samples(self, which=("T", "z", "p"), compact=True):
        """-> dict name -> (S, M) array (M = surviving rays when `compact`, else all N; dropped rays are NaN then)."""
        if self.M is None:
            self.wait()
        cols = self.M if compact else self.N
        bufs = {k: (np.empty((self.S, self.N)) if k in which else None) for k in ("T", "z", "p")}
        check(load().pgr_fan_fetch_samples(self._h, _addr(bufs["T"]), _addr(bufs["z"]), _addr(bufs["p"]),
                                           PGR_COMPACT if compact else 0))
        return {k: (v.reshape(-1)[:self.S * cols].reshape(self.S, cols) if cols != self.N else v)
                for k, v in bufs.items() if v is not None}

    def close(self):
        if getattr(self, "_h", None):
            load().pgr_fan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def initial_states_device(device, ang_ptr, n, source_depth, c_source, y0_ptr, stream=0):
    """pgr_initial_states_device on raw device pointers (ints)."""
    check(load().pgr_initial_states_device(int(device), ang_ptr, int(n), float(source_depth), float(c_source), y0_ptr, stream))


def debug_math(a, b):
    a = _c(a); b = _c(b)
    out = np.empty((len(a), 9))
    check(load().pgr_debug_math(_addr(a), _addr(b), len(a), _addr(out)))
    return out


def device_count():
    return load().pgr_device_count()


def build_info():
    """pgr_build_info(): layout pass applied or not + arithmetic variant of the loaded library."""
    return load().pgr_build_info().decode()


def device_code_sha256(path=None):
    """sha256 of the gfx950 machine code (.text of the code object inside the library's fat binary): what the
    kernels ARE, independent of symbol order and build paths (two builds of the same source give the same hash).
    profiles/*_traffic.json records it next to the counters; bench.py reports counters only for the code they
    were taken with."""
    import hashlib
    import struct

    def sections(b):
        shoff = struct.unpack_from("<Q", b, 0x28)[0]
        shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)
        secs = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize) for i in range(shnum)]
        stro = secs[shstrndx][4]
        return {b[stro + s_[0]:b.index(b"\0", stro + s_[0])].decode(): (s_[4], s_[5]) for s_ in secs}

    with open(path or LIB_PATH, "rb") as f:
        b = f.read()
    o, n = sections(b)[".hip_fatbin"]
    fb = b[o:o + n]
    if fb[:24] != b"__CLANG_OFFLOAD_BUNDLE__":
        raise PgrError("unexpected fat binary layout")
    cnt = struct.unpack_from("<Q", fb, 24)[0]
    p = 32
    for _ in range(cnt):
        off, size, tl = struct.unpack_from("<QQQ", fb, p)
        p += 24
        triple = fb[p:p + tl].decode()
        p += tl
        if "gfx950" in triple:
            elf = fb[off:off + size]
            to, tn = sections(elf)[".text"]
            return hashlib.sha256(elf[to:to + tn]).hexdigest()
    raise PgrError("no gfx950 code object in the library")


def arrival_histogram_device(device, t_ptr, t_stride, status_ptr, status_stride, n, t_min, t_max, nbins,
                             counts_ptr, stream=0):
    """pgr_arrival_histogram_device on raw device pointers (ints); see include/pgr.h."""
    check(load().pgr_arrival_histogram_device(int(device), t_ptr, int(t_stride), status_ptr, int(status_stride), int(n),
                                              float(t_min), float(t_max), int(nbins), counts_ptr, stream))


def intensity_device(env, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, depths_ptr, n_depths, out_ptr, stream=0,
                     weights=0):
    """pgr_intensity_device on raw device pointers (ints): the ray-tube intensity of caller buffers z / p [n_samples][n_rays]
    (stored sign convention) on `env` (an EnvHandle); see include/pgr.h.  `weights` (here and in beam_intensity_device /
    arrivals_device): a device pointer to [n_samples][n_rays] weights of g, which selects the entry's weighted twin
    (pgr_intensity_device_w); 0: the unweighted entry."""
    _buffers(env, n_rays, n_samples, x_ptr, z_ptr, p_ptr).intensity(p0_ptr, depths_ptr, n_depths, out_ptr, stream, weights)


def beam_intensity_device(env, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, bottom_ptr, depths_ptr, n_depths, min_width,
                          out_ptr, stream=0, weights=0):
    """pgr_beam_intensity_device on raw device pointers (ints): the Gaussian-beam intensity of caller buffers z / p
    [n_samples][n_rays] (stored sign convention) on `env` (an EnvHandle); see include/pgr.h."""
    _buffers(env, n_rays, n_samples, x_ptr, z_ptr, p_ptr).beam_intensity(p0_ptr, bottom_ptr, depths_ptr, n_depths, min_width,
                                                                         out_ptr, stream, weights)


def arrival_counts_device(env, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, depths_ptr, n_depths, cols, counts_ptr,
                          stream=0):
    """pgr_arrival_counts_device on raw device pointers (ints) of caller buffers z / p [n_samples][n_rays] (stored sign
    convention) on `env` (an EnvHandle); `cols` a host sequence of column indices; see include/pgr.h."""
    _buffers(env, n_rays, n_samples, x_ptr, z_ptr, p_ptr).arrival_counts(p0_ptr, depths_ptr, n_depths, cols, counts_ptr, stream)


def arrivals_device(env, t_ptr, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, depths_ptr, n_depths, cols, offsets_ptr,
                    n_arrivals, tube_ptr, w_ptr, t_out_ptr, p_out_ptr, i_ptr, stream=0, weights=0):
    """pgr_arrivals_device on raw device pointers (ints): arrival_counts_device's walk, writing the arrivals; see
    include/pgr.h."""
    _buffers(env, n_rays, n_samples, x_ptr, t_ptr, z_ptr, p_ptr).arrivals(
        p0_ptr, depths_ptr, n_depths, cols, offsets_ptr, n_arrivals, tube_ptr, w_ptr, t_out_ptr, p_out_ptr, i_ptr, stream, weights)


def travel_time_kernel_device(env, t_ptr, z_ptr, n_rays, n_samples, x_ptr, ranges_ptr, n_ranges, depths_ptr, n_depths,
                              column, out_ptr, stream=0):
    """pgr_travel_time_kernel_device on raw device pointers (ints): the travel-time sensitivity kernel of caller buffers
    T / z [n_samples][n_rays] (stored sign convention) on `env` (an EnvHandle); see include/pgr.h."""
    _buffers(env, n_rays, n_samples, x_ptr, t_ptr, z_ptr).travel_time_kernel(ranges_ptr, n_ranges, depths_ptr, n_depths, column,
                                                                             out_ptr, stream)


def time_front_device(device, t_ptr, z_ptr, p_ptr, n_rays, n_samples, cols, t_out_ptr, z_out_ptr, p_out_ptr, turns_ptr,
                      stream=0):
    """pgr_time_front_device on raw device pointers (ints; 0 / None: absent): the samples at the save columns `cols` (a
    host sequence, or None for a NULL list) and the turning-point counts up to them, of caller buffers T / z / p
    [n_samples][n_rays] on `device`; see include/pgr.h."""
    _Buffers(int(device), t_ptr, z_ptr, p_ptr, int(n_rays), int(n_samples)).time_front(cols, t_out_ptr, z_out_ptr, p_out_ptr,
                                                                                     turns_ptr, stream)


def path_integral_device(env, t_ptr, z_ptr, n_rays, n_samples, x_ptr, a_depths, alpha, out_ptr, stream=0):
    """pgr_path_integral_device on raw device pointers (ints): out[n_samples][n_rays] = the running path integral of caller
    buffers T / z [n_samples][n_rays] (stored sign convention) on `env` (an EnvHandle) for the absorption profile alpha
    (dB/m) on the depth nodes a_depths (host sequences; a_depths None with one alpha); see include/pgr.h."""
    _buffers(env, n_rays, n_samples, x_ptr, t_ptr, z_ptr).path_integral(a_depths, alpha, out_ptr, stream)


def boundary_tables(bottom, surface, beta):
    """Three (nodes or None, values) pairs -> the host arrays pgr_fan_boundary_loss / pgr_boundary_loss_device take (kept
    alive by the returned tuple): the bottom loss on grazing angles, the surface loss, the bottom slope in degrees on ranges."""
    return tuple(_profile(nodes, values, "a table's nodes and values") for nodes, values in (bottom, surface, beta))


def _table_args(tables):
    args = []
    for x, v in tables:
        args += [_addr(x), _addr(v), len(v)]
    return args


def boundary_loss_device(env, bx_ptr, bp_ptr, bk_ptr, n_rays, K, x0, x1, n_samples, tables, out_ptr, nb_ptr=0, ns_ptr=0,
                         stream=0):
    """pgr_boundary_loss_device on raw device pointers (ints): the log bx, bp (float64) and bk (int8), [K][n_rays] each, stored
    sign, on the save ranges np.linspace(x0, x1, n_samples) of the frame of `env`."""
    _Buffers(env._h, bx_ptr, bp_ptr, bk_ptr, int(n_rays), int(K), float(x0), float(x1), int(n_samples)).boundary_loss(
        tables, out_ptr, nb_ptr, ns_ptr, stream)


def absorption_weights_device(device, a_ptr, n, w_ptr, stream=0):
    """pgr_absorption_weights_device on raw device pointers (ints): W[i] = 10^(-A[i] / 10) for n path integrals in dB (W may
    be A); see include/pgr.h."""
    check(load().pgr_absorption_weights_device(int(device), a_ptr, int(n), w_ptr, stream))


def caustic_index_device(device, z_ptr, n_rays, n_samples, nb_ptr, ns_ptr, kappa_ptr, stream=0):
    """pgr_caustic_index_device on raw device pointers (ints; nb / ns 0: absent): kappa[n_samples][n_rays] int32 of caller rows
    z [n_samples][n_rays] (stored sign convention) on `device`; see include/pgr.h."""
    _Buffers(int(device), z_ptr, int(n_rays), int(n_samples)).caustic_index(nb_ptr, ns_ptr, kappa_ptr, stream)


def pressure_device(env, t_ptr, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, q_ptr, frequency, depths_ptr, n_depths, re_ptr,
                    im_ptr, stream=0, weights=0):
    """pgr_pressure_device_w on raw device pointers (ints; q / weights 0: absent): the coherent tube sum of caller buffers
    T / z / p [n_samples][n_rays] (stored sign convention) on `env` (an EnvHandle); see include/pgr.h."""
    _buffers(env, n_rays, n_samples, x_ptr, t_ptr, z_ptr, p_ptr).pressure(p0_ptr, q_ptr, frequency, depths_ptr, n_depths, re_ptr,
                                                                          im_ptr, stream, weights)


def pressure_phi_device(env, t_ptr, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, q_ptr, phi_ptr, frequency, depths_ptr,
                        n_depths, re_ptr, im_ptr, stream=0, weights=0):
    """pgr_pressure_device_phi on raw device pointers (ints): ``pressure_device`` with phi [n_samples][n_rays] float64, the
    rays' lag in cycles (include/pgr_reflection.h); phi 0 is refused."""
    _buffers(env, n_rays, n_samples, x_ptr, t_ptr, z_ptr, p_ptr).pressure_phi(p0_ptr, q_ptr, phi_ptr, frequency, depths_ptr,
                                                                              n_depths, re_ptr, im_ptr, stream, weights)


def beam_pressure_device(env, t_ptr, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, q_ptr, frequency, bottom_ptr, depths_ptr,
                         n_depths, min_width, curvature, re_ptr, im_ptr, stream=0, weights=0):
    """pgr_beam_pressure_device_w on raw device pointers (ints; q / weights 0: absent): the coherent Gaussian-beam sum of caller
    buffers T / z / p [n_samples][n_rays] (stored sign convention) on `env` (an EnvHandle); see include/pgr_beam_coherent.h."""
    _buffers(env, n_rays, n_samples, x_ptr, t_ptr, z_ptr, p_ptr).beam_pressure(
        p0_ptr, q_ptr, frequency, bottom_ptr, depths_ptr, n_depths, min_width, curvature, re_ptr, im_ptr, stream, weights)


def beam_arrival_counts_device(env, t_ptr, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, q_ptr, bottom_ptr, depths_ptr,
                               n_depths, min_width, cols, counts_ptr, stream=0, weights=0):
    """pgr_beam_arrival_counts_device_w on raw device pointers (ints; q / weights 0: absent): the terms ``beam_pressure_device``
    adds per receiver depth and requested column of `cols` (a host sequence), of caller buffers T / z / p [n_samples][n_rays]
    (stored sign convention) on `env` (an EnvHandle); see include/pgr_beam_arrivals.h."""
    _buffers(env, n_rays, n_samples, x_ptr, t_ptr, z_ptr, p_ptr).beam_arrival_counts(
        p0_ptr, q_ptr, bottom_ptr, depths_ptr, n_depths, min_width, cols, counts_ptr, stream, weights)


def beam_arrivals_device(env, t_ptr, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, q_ptr, bottom_ptr, depths_ptr, n_depths,
                         min_width, cols, curvature, offsets_ptr, n_arrivals, tube_ptr, image_ptr, time_ptr, amp_ptr, qa_ptr,
                         stream=0, weights=0):
    """pgr_beam_arrivals_device_w on raw device pointers (ints): beam_arrival_counts_device's walk, writing the arrivals; see
    include/pgr_beam_arrivals.h."""
    _buffers(env, n_rays, n_samples, x_ptr, t_ptr, z_ptr, p_ptr).beam_arrivals(
        p0_ptr, q_ptr, bottom_ptr, depths_ptr, n_depths, min_width, cols, curvature, offsets_ptr, n_arrivals, tube_ptr, image_ptr,
        time_ptr, amp_ptr, qa_ptr, stream, weights)


def _signal(suffix, device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, phi, tstart_ptr, frequency, inv_sigma, dt, n_times,
            re_ptr, im_ptr, stream):
    """pgr_signal_device`suffix`; `phi`: the pointers the entry takes between q and tstart: () or (phi_ptr,)"""
    check(getattr(load(), "pgr_signal_device" + suffix)(
        int(device), offsets_ptr, int(n_groups), t_ptr, i_ptr, q_ptr or None, *(p or None for p in phi), tstart_ptr,
        float(frequency), float(inv_sigma), float(dt), int(n_times), re_ptr, im_ptr, stream))


def signal_device(device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, tstart_ptr, frequency, inv_sigma, dt, n_times, re_ptr,
                  im_ptr, stream=0):
    """pgr_signal_device on raw device pointers (ints; q 0: absent): re / im [n_groups][n_times] = the complex baseband signal
    of a Gaussian pulse (inv_sigma = 1 / sigma; 0: CW) summed over the arrivals T / I / q of each group [offsets[g],
    offsets[g + 1]) at the times tstart[g] + n dt; see include/pgr_signal.h."""
    _signal("", device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, (), tstart_ptr, frequency, inv_sigma, dt, n_times, re_ptr,
            im_ptr, stream)


def signal_phi_device(device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, phi_ptr, tstart_ptr, frequency, inv_sigma, dt, n_times,
                      re_ptr, im_ptr, stream=0):
    """pgr_signal_device_phi on raw device pointers (ints): ``signal_device`` with phi float64, every arrival's lag in cycles
    (include/pgr_reflection.h); phi 0 is refused."""
    _signal("_phi", device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, (phi_ptr,), tstart_ptr, frequency, inv_sigma, dt, n_times,
            re_ptr, im_ptr, stream)


def array_response_sum(device, offsets_ptr, n_elements, n_cols, t_ptr, i_ptr, q_ptr, phi_ptr, delay_ptr, weight_ptr, tstart_ptr,
                       frequency, inv_sigma, dt, n_times, n_looks, re_ptr, im_ptr, stream=0):
    """pgr_array_response_device on raw device pointers (ints; q / phi 0: absent): re / im [n_cols][n_looks][n_times] = the
    delay-and-sum of the arrivals T / I / q / phi of the groups g = j * n_cols + c over the n_elements elements j, with the
    delays delay[g][n_looks] and the weights weight[g], at the times tstart[c] + n dt; see include/pgr_array.h.  (Named
    after what it does, not `..._device`: it has no fan-handle twin.)"""
    check(load().pgr_array_response_device(
        int(device), offsets_ptr, int(n_elements), int(n_cols), t_ptr, i_ptr, q_ptr or None, phi_ptr or None, delay_ptr,
        weight_ptr, tstart_ptr, float(frequency), float(inv_sigma), float(dt), int(n_times), int(n_looks), re_ptr, im_ptr, stream))


def _spectrum(suffix, device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, phi, l_ptr, tred_ptr, freq, alpha, re_ptr, im_ptr,
              stream):
    """pgr_spectrum_device`suffix`; `phi`: the pointers the entry takes between q and l: () or (phi_ptr,)"""
    al, fr = _profile(alpha, freq, "freq and alpha")
    check(getattr(load(), "pgr_spectrum_device" + suffix)(
        int(device), offsets_ptr, int(n_groups), t_ptr, i_ptr, q_ptr or None, *(p or None for p in phi), l_ptr or None, tred_ptr,
        _addr(fr), _addr(al), len(fr), re_ptr, im_ptr, stream))


def spectrum_device(device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, l_ptr, tred_ptr, freq, alpha, re_ptr, im_ptr,
                    stream=0):
    """pgr_spectrum_device on raw device pointers (ints; q / l 0: absent) and the HOST sequences freq (Hz) and alpha (dB per
    metre, or None; given exactly when l is): re / im [n_groups][len(freq)] = the transfer function of the arrivals T / I / q
    / L of each group [offsets[g], offsets[g + 1]) at every frequency, reduced by tred[g]; see include/pgr_spectrum.h."""
    _spectrum("", device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, (), l_ptr, tred_ptr, freq, alpha, re_ptr, im_ptr, stream)


def spectrum_phi_device(device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, phi_ptr, l_ptr, tred_ptr, freq, alpha, re_ptr, im_ptr,
                        stream=0):
    """pgr_spectrum_device_phi on raw device pointers (ints) and the HOST sequences freq and alpha: ``spectrum_device`` with phi
    float64, every arrival's lag in cycles (include/pgr_reflection.h); phi 0 is refused."""
    _spectrum("_phi", device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, (phi_ptr,), l_ptr, tred_ptr, freq, alpha, re_ptr, im_ptr,
              stream)


def band_power_sum(device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, phi_ptr, l_ptr, freq, alpha, weights, out_ptr, stream=0):
    """pgr_band_power_device on raw device pointers (ints; q / phi / l 0: absent) and the HOST sequences freq (Hz), alpha (dB per
    metre, or None; given exactly when l is) and weights (one per frequency, finite and >= 0): out [n_groups] = the power of the
    arrivals T / I / q / phi / L of each group [offsets[g], offsets[g + 1]) summed over the band, sum_k weights[k] |H(freq[k])|^2
    in the order of include/pgr_band.h.  (Named after what it does, not `..._device`: it has no fan-handle twin.)"""
    al, fr = _profile(alpha, freq, "freq and alpha")
    _, wf = _profile(None, weights, "weights")
    if len(wf) != len(fr):
        raise ValueError("freq and weights must have equal length")
    check(load().pgr_band_power_device(
        int(device), offsets_ptr, int(n_groups), t_ptr, i_ptr, q_ptr or None, phi_ptr or None, l_ptr or None, _addr(fr), _addr(al),
        _addr(wf), len(fr), out_ptr, stream))


def matched_field_sum(device, offsets_ptr, n_elements, n_cells, t_ptr, i_ptr, q_ptr, phi_ptr, l_ptr, freq, alpha, weights, data,
                      normalize, out_ptr, stream=0):
    """pgr_matched_field_device on raw device pointers (ints; q / phi / l 0: absent) and the HOST sequences freq (Hz), alpha (dB
    per metre, or None; given exactly when l is), weights (one per frequency, finite and >= 0) and data (complex, (n_elements,
    len(freq)), finite): out [n_cells] = the Bartlett power of the data against the replicas of every cell, formed from the
    arrivals T / I / q / phi / L of the groups j * n_cells + g over the elements j and summed over the band in the order of
    include/pgr_match.h; `normalize`: divided by the replicas' squared norm per frequency.  (Named after what it does, not
    `..._device`: it has no fan-handle twin.)"""
    al, fr = _profile(alpha, freq, "freq and alpha")
    _, wf = _profile(None, weights, "weights")
    if len(wf) != len(fr):
        raise ValueError("freq and weights must have equal length")
    d = np.asarray(data, dtype=np.complex128)
    if d.shape != (int(n_elements), len(fr)):
        raise ValueError("data must hold one complex value per element and frequency")
    dr, di = _c(d.real), _c(d.imag)
    check(load().pgr_matched_field_device(
        int(device), offsets_ptr, int(n_elements), int(n_cells), t_ptr, i_ptr, q_ptr or None, phi_ptr or None, l_ptr or None,
        _addr(fr), _addr(al), _addr(wf), _addr(dr), _addr(di), len(fr), int(bool(normalize)), out_ptr, stream))
