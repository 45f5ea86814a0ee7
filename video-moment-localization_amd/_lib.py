"""ctypes binding of libsmin_hip.so (C ABI: include/smin_hip.h).  No CPU fallback: every entry point
raises if the library is missing or a tensor is not on a HIP device."""
import ctypes
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsmin_hip.so")
TORCH_LIB_PATH = os.path.join(_HERE, "libsmin_torch.so")        # TORCH_LIBRARY(smin_hip, ...): csrc/torch_binding.cpp
CSRC = os.path.join(_HERE, "csrc")

HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "smin_hip.h")  # where csrc/Makefile finds it (-I../../include)
ABI_VERSION = 2                                                 # include/smin_hip.h SMIN_HIP_ABI_VERSION

_SCALARS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double, "int64_t": ctypes.c_int64}


class SminHipError(RuntimeError):
    pass


def _parse_header(text):
    """({name: argtypes}, {name: restype, where it is not int}) of every `int | size_t | const char* smin_*(...);` prototype of a
    C header: any pointer is a c_void_p, the scalars are _SCALARS, (void) is no argument."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    signatures, restypes = {}, {}
    for ret, name, args in re.findall(r"\b(int|size_t|const\s+char\s*\*)(?:(?<=\*)|\s)\s*(smin_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        row = []
        for arg in ([] if args.strip() in ("", "void") else args.split(",")):
            ty = " ".join(re.sub(r"\bconst\b", " ", arg).split()[:-1])     # the last word is the argument's name
            if "*" not in arg and ty not in _SCALARS:
                raise SminHipError(f"{name}: no ctypes type for the argument `{' '.join(arg.split())}`")
            row.append(ctypes.c_void_p if "*" in arg else _SCALARS[ty])
        signatures[name] = row
        if ret != "int":
            restypes[name] = ctypes.c_size_t if ret == "size_t" else ctypes.c_char_p
    return signatures, restypes


def _header_table():
    if not os.path.exists(HEADER_PATH):
        raise SminHipError(f"{HEADER_PATH} is missing: the ctypes table is read from the C header")
    with open(HEADER_PATH) as f:
        return _parse_header(f.read())


# name -> argtypes (restype is int unless listed in _RESTYPE): include/smin_hip.h, read at import
SIGNATURES, _RESTYPE = _header_table()

_lib = None
_ws = {}


def build(verbose=False):
    """Compile every HIP source for gfx950 into libsmin_hip.so (hipcc cross-compiles without a GPU)."""
    res = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode != 0:
        raise SminHipError("building libsmin_hip.so failed (see output above)")
    return LIB_PATH


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SminHipError(
            f"{LIB_PATH} is missing: the SMIN hot path has no CPU fallback. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc, --offload-arch=gfx950).")
    lib = ctypes.CDLL(LIB_PATH)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here == header/library mismatch
        fn.argtypes = args
        fn.restype = _RESTYPE.get(name, ctypes.c_int)
    if lib.smin_abi_version() != ABI_VERSION:
        raise SminHipError("libsmin_hip.so ABI version mismatch")
    _lib = lib
    if DEFAULT_GEMM_MODE != "f32":                        # deployment switch: SMIN_GEMM_MODE=f32e|bf16x3|bf16 (see set_gemm_mode)
        check(lib.smin_set_gemm_mode(GEMM_MODES[DEFAULT_GEMM_MODE]), "smin_set_gemm_mode")
    return lib


_torch_ops = None


def load_torch():
    """The torch-extension binding (csrc/torch_binding.cpp): registers torch.ops.smin_hip.{smin_forward, smin_score, smin_loss, adam_step,
    smin_encode_videos, smin_encode_queries, smin_score_pairs, smin_score_pairs_compact, smin_corpus_span_topk, smin_forward_pairs, smin_pair_rank_loss, smin_pair_distill_loss} -- the whole forward as one library call with its autograd graph built in
    C++, its forward-only scoring twin, the optimizer step over a parameter list, the corpus-search operators (the two encoders
    alone, the scorer over indexed pairs of their banks, the ranking of span-valued moments across videos) and the contrastive and soft-target terms over a pair plan.  Raises if the library is missing."""
    global _torch_ops
    if _torch_ops is not None:
        return _torch_ops
    load()                                            # the C ABI library it links against
    if not os.path.exists(TORCH_LIB_PATH):
        raise SminHipError(
            f"{TORCH_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or set SMIN.fused_core = False to drive the same kernels from the Python host)")
    torch.ops.load_library(TORCH_LIB_PATH)
    ops = torch.ops.smin_hip
    if ops.abi_version() != ABI_VERSION:
        raise SminHipError("libsmin_torch.so / libsmin_hip.so ABI version mismatch")
    _torch_ops = ops
    return ops


def ptr(t):
    """Device pointer of a contiguous HIP tensor of one of the element types the C ABI takes (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise SminHipError("the SMIN hot path runs on a HIP device only (got a CPU tensor); there is no CPU fallback")
    if not t.is_contiguous():
        raise SminHipError("internal error: non-contiguous tensor handed to the C ABI")
    if t.dtype not in (torch.float32, torch.int32, torch.uint8, torch.float64, torch.bool, torch.int64, torch.bfloat16, torch.int8):
        raise SminHipError(f"unsupported dtype {t.dtype}")
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(nbytes, device):
    """Persistent scratch buffer per (device, stream), grown on demand: calls on one stream are stream-ordered, and
    units running side by side on two streams never share scratch.  Inside a stream capture the scratch is a fresh tensor of the
    graph's own memory pool: a captured graph keeps the pointer it is given, and the persistent buffer is replaced by the next larger
    request."""
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
        _ws[key] = buf
    return buf


def check(rc, name):
    if rc != 0:
        raise SminHipError(f"{name} failed with code {rc}" + (" (argument rejected at csrc line %d)" % (-rc - 1000) if rc < -1000 else ""))


def call(name, *args):
    check(getattr(load(), name)(*args), name)


def call_ws(name, size_args, *args, query=None, fields=None):
    """``call(name, *args, ws, ws_bytes)`` with a fresh workspace on the current device, sized by the entry point's own query
    (``name + "_ws_bytes"`` unless ``query`` names another) at ``size_args``.  A size of 0 is the query's refusal of its arguments:
    the error names the query and the arguments, by ``fields`` ("B, L, k") where the caller gives their names."""
    query = query or name + "_ws_bytes"
    nbytes = getattr(load(), query)(*size_args)
    if nbytes == 0:
        named = ", ".join(f"{f}={v}" for f, v in zip(fields.split(", "), size_args)) if fields else tuple(size_args)
        raise SminHipError(f"{query} rejected {named}")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    call(name, *args, ptr(ws), nbytes)


PROF_TAGS = {1: "moment_fwd", 2: "moment_dx", 3: "moment_dw", 4: "attn_fwd", 5: "attn_bwd"}


def prof_enable(on=True):
    """Bracket the tagged launches (include/smin_hip.h SMIN_PROF_*) with HIP events on their launch stream."""
    check(load().smin_prof_enable(int(on)), "smin_prof_enable")


def prof_read(cap=1 << 16):
    """{tag name: [milliseconds per launch, in launch order]} of everything recorded since prof_enable(True)."""
    tags, ms = (ctypes.c_int32 * cap)(), (ctypes.c_float * cap)()
    n = load().smin_prof_read(tags, ms, cap)
    if n < 0:
        raise SminHipError(f"smin_prof_read failed with code {n}")
    out = {}
    for k in range(n):
        out.setdefault(PROF_TAGS.get(tags[k], str(tags[k])), []).append(ms[k])
    return out


GEMM_MODES = {"f32": 0, "bf16x3": 1, "bf16": 2, "f32e": 3}
DEFAULT_GEMM_MODE = os.environ.get("SMIN_GEMM_MODE", "f32")      # the mode the library starts in (and tests restore)
if DEFAULT_GEMM_MODE not in GEMM_MODES:
    raise ValueError(f"SMIN_GEMM_MODE={DEFAULT_GEMM_MODE!r}: expected one of {sorted(GEMM_MODES)}")


def set_gemm_mode(mode):
    """Arithmetic of the dense contractions (forward, input gradients, weight gradients): "f32" (exact fp32 MFMA, default),
    "f32e" (fp32 emulated on the bf16 matrix cores: exact three-way bf16 split of each operand, six products, fp32 accumulation --
    agrees with "f32" to fp32 rounding), "bf16x3" (two-way split, three products; ~1e-5 relative) or "bf16" (operands rounded to
    bf16 once; ~4e-3 relative per product -- BASELINE.json configs[1])."""
    check(load().smin_set_gemm_mode(GEMM_MODES[mode]), "smin_set_gemm_mode")


def get_gemm_mode():
    m = load().smin_get_gemm_mode()
    return [k for k, v in GEMM_MODES.items() if v == m][0]
