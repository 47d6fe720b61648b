"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol
include/conmamba_hip.h declares; argument validation works without a GPU."""
import ctypes as C
import keyword
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    import mamba_asr_amd._native as N
    if not os.path.exists(N.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "mamba_asr_amd", "csrc")])
    return N


def test_header_symbols_exported(native):
    hdr = open(os.path.join(ROOT, "include", "conmamba_hip.h")).read()
    hdr = re.sub(r"#ifdef CM_ABLATE.*?#endif", "", hdr, flags=re.S)      # the ablation build's switch is not part of the product ABI
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char \*)\s*\*?\s*(cm_[a-z0-9_]+)\s*\(", hdr, re.M))
    assert {"cm_selective_scan_fwd", "cm_selective_scan_bwd", "cm_causal_conv1d_fwd", "cm_causal_conv1d_bwd",
            "cm_abi_version", "cm_last_error", "cm_scan_num_chunks", "cm_scan_cl_fwd", "cm_conv_cl_fwd", "cm_conv_xproj", "cm_fbank_wav", "cm_cnn_front", "cm_ln_pw_glu", "cm_dwconv1d_fwd", "cm_dwconv1d_bwd", "cm_dwconv_cl_fwd", "cm_dwconv_cl_bwd", "cm_dwconv_cl_workspace_floats", "cm_causal_conv1d_update", "cm_selective_state_update", "cm_add_layernorm", "cm_layernorm_fwd", "cm_layernorm_bwd", "cm_layernorm_bwd_workspace_floats",
            "cm_glu_dwconv_ln_gelu", "cm_cnn_block1", "cm_gemm_bf16", "cm_fbank_mel_db", "cm_fbank_finish",
            "cm_spec_drop"} <= declared
    handle = C.CDLL(native.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in conmamba_hip.h but not exported"
    assert {s[0] for s in native.SYMBOLS} == declared
    # the product library carries no process-global switch (ablation variants live in the CM_ABLATE build only)
    for name in ("cm_debug_set", "cm_debug_get", "cm_scan_set_split"):
        assert not hasattr(handle, name), f"{name} must not be exported by the product library"


def _host_cc():
    """$CC, else cc, else the clang that ships beside hipcc: the first that runs."""
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    beside = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "clang")
    tried = [c for c in (os.environ.get("CC"), "cc", beside) if c]
    for cc in tried:
        try:
            if subprocess.run(cc.split() + ["--version"], capture_output=True).returncode == 0:
                return cc.split()
        except OSError:
            pass
    pytest.fail(f"no host C compiler runs (tried {tried}): the library cannot be built here either")


def test_struct_layouts_match_the_compiler(native, tmp_path):
    """Every derived ctypes class against the C compiler's own sizeof / offsetof of the real header: the size of every
    struct, the offset and size of every field (pad words included)."""
    hdr = open(os.path.join(ROOT, "include", "conmamba_hip.h")).read()
    structs = native.HEADER.structs
    assert set(structs) == set(re.findall(r"^typedef\s+struct\s+(\w+)\s*\{", hdr, re.M)) and len(structs) >= 38
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "conmamba_hip.h"', 'int main(void) {']
    want = []
    for cname, cls in structs.items():
        src.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        want.append(f"{cname} {C.sizeof(cls)}")
        for field, _ in cls._fields_:
            cfield = field[:-1] if field.endswith("_") and keyword.iskeyword(field[:-1]) else field      # in_ is C's `in`
            src.append(f'    printf("{cname}.{cfield} %zu %zu\\n", offsetof({cname}, {cfield}), sizeof((({cname} *)0)->{cfield}));')
            want.append(f"{cname}.{cfield} {getattr(cls, field).offset} {getattr(cls, field).size}")
    src += ['    return 0;', '}', '']
    (tmp_path / "probe.c").write_text("\n".join(src))
    subprocess.check_call(_host_cc() + ["-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")])
    got = subprocess.check_output([str(tmp_path / "probe")], text=True).splitlines()
    assert len(got) == len(want) > 600
    assert [g for g, w in zip(got, want) if g != w] == [], "compiler (left in the list) and ctypes disagree"
    assert native.LayerNormArgs is structs["cm_layernorm_args"] and native.ScanClDir is structs["cm_scan_cl_dir"]
    assert hasattr(native.GluDwconvArgs, "in_") and not hasattr(native.GluDwconvArgs, "in")
    assert native.ABI_VERSION == native.CM_ABI_VERSION == int(re.search(r"#define CM_ABI_VERSION (\d+)", hdr).group(1))
    assert native.CM_SEED_EPOCH_MUL == 0x9E3779B97F4A7C15 and native.CM_EALIGN == -3 and native.CM_BF16 == 1


@pytest.mark.parametrize("snippet, quoted", [
    ("typedef struct cm_t { int32_t a; unsigned short x; } cm_t;", "unsigned short x"),              # unknown base type
    ("typedef struct cm_t { int32_t a; size_t n; } cm_t;", "size_t n"),
    ("typedef struct cm_t { const foo_t *p; } cm_t;", "foo_t *p"),                                   # unknown pointee
    ("typedef struct cm_t { int32_t flag : 1; int32_t rest : 31; } cm_t;", "int32_t flag : 1"),      # bit-field
    ("typedef struct cm_t { int32_t kind; union { int32_t i; float f; } u; } cm_t;", "union {"),     # union member
    ("typedef union cm_u { int32_t i; float f; } cm_u;", "typedef union cm_u"),
    ("typedef struct cm_t { void *ctx; int (*callback)(void *); } cm_t;", "int (*callback)(void *)"),   # function pointer
    ("typedef struct cm_t { int32_t a; } cm_other;", "cm_other"),
    ("typedef struct cm_t { void * const p; } cm_t;", "void * const p"),
    ("#if defined(CM_WIDE)\ntypedef struct cm_t { int64_t a; } cm_t;\n#endif", "#if defined(CM_WIDE)"),     # stray conditional
    ("#ifdef CM_OTHER\nint cm_f(void);\n#endif", "#ifdef CM_OTHER"),
    ("#ifdef CM_ABLATE\n#else\nint cm_f(void);\n#endif", "#else"),
    ("#define CM_X (1 << 4)", "#define CM_X (1 << 4)"),
    ("#define CM_MAX(a, b) ((a) > (b) ? (a) : (b))", "#define CM_MAX(a, b)"),
    ("typedef enum { CM_A = 0, CM_B } cm_e;", "CM_B"),
    ("float cm_f(int32_t n);", "float cm_f(int32_t n)"),                                             # return type outside the list
    ("int cm_f(size_t n);", "int cm_f(size_t n)"),
    ("int cm_f(int32_t n)", "int cm_f(int32_t n)"),                                                  # no terminator
    ("int cm_f(void);\nint cm_f(void);", "int cm_f(void)"),
    ("static const int cm_k = 3;", "static const int cm_k = 3"),
])
def test_parser_refuses_what_it_does_not_understand(native, snippet, quoted):
    with pytest.raises(ValueError, match=re.escape(quoted)):
        native.parse_header(snippet)


def test_parser_reads_the_supported_forms(native):
    h = native.parse_header("""
        /* a block comment; with, separators */
        #ifndef CM_T_H
        #define CM_T_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define CM_T_VERSION 3
        #define CM_T_NEG   (-2)   // trailing; comment, too
        #define CM_T_BIG 0x9E3779B97F4A7C15ull
        typedef enum { CM_T_A = 0, CM_T_B = 0x10 } cm_t_kind;
        typedef struct cm_t_dir {
            const float *w;       /* a comment; holding , and ; */
            int64_t bs, ts;
            int32_t rank;         // one; more, of them
        } cm_t_dir;
        typedef struct cm_t_args {
            int32_t n;
            cm_t_dir dir[2];
            uint64_t hash_base[2], hash_sep;
            double scale;
            const void *in;
            float *a, *b;
            uint8_t *mask;
            cm_t_dir *one;
            int last;
        } cm_t_args;
        int cm_t_run(const cm_t_args *args);
        int64_t cm_t_pack(const void *w /* (rows, cols); packed */, int32_t rows,
                          int32_t cols,   // cols, then the stream
                          void *stream);
        const char *cm_t_error(void);
        #ifdef CM_ABLATE
        int cm_t_debug(int which);
        #endif
        #ifdef __cplusplus
        }
        #endif
        #endif
        """)
    assert h.consts == {"CM_T_VERSION": 3, "CM_T_NEG": -2, "CM_T_BIG": 0x9E3779B97F4A7C15, "CM_T_A": 0, "CM_T_B": 16}
    assert list(h.structs) == ["cm_t_dir", "cm_t_args"]
    D, A = h.structs["cm_t_dir"], h.structs["cm_t_args"]
    assert (D.__name__, A.__name__) == ("TDir", "TArgs")

    def layout(cls):
        return [(n, getattr(cls, n).offset, getattr(cls, n).size) for n, _ in cls._fields_]
    assert layout(D) == [("w", 0, 8), ("bs", 8, 8), ("ts", 16, 8), ("rank", 24, 4)] and C.sizeof(D) == 32
    assert layout(A) == [("n", 0, 4), ("dir", 8, 64), ("hash_base", 72, 16), ("hash_sep", 88, 8), ("scale", 96, 8), ("in_", 104, 8),
                         ("a", 112, 8), ("b", 120, 8), ("mask", 128, 8), ("one", 136, 8), ("last", 144, 4)] and C.sizeof(A) == 152
    t = dict(A._fields_)
    assert t["dir"] is D * 2 and t["hash_base"] is C.c_uint64 * 2 and t["scale"] is C.c_double and t["last"] is C.c_int
    assert all(t[k] is C.c_void_p for k in ("in_", "a", "b", "mask", "one"))
    assert h.protos == {"cm_t_run": (C.c_int, [C.POINTER(A)]),
                        "cm_t_pack": (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
                        "cm_t_error": (C.c_char_p, [])}
    assert h.ablate_protos == {"cm_t_debug": (C.c_int, [C.c_int])}


def test_store_to_a_name_that_is_no_field_raises(native):
    a = native.ScanFwdArgs()
    a.seqlen = 5                                    # a field: stored
    assert a.seqlen == 5
    with pytest.raises(AttributeError):
        a.no_such_field = 1
    s = native.ScanClArgs()
    s.dir[0].xdbl_ts = 7
    assert s.dir[0].xdbl_ts == 7
    with pytest.raises(AttributeError):
        s.dir[0].xdlb_ts = 7                        # the typo that used to leave the C field zero
    for cls in native.HEADER.structs.values():
        assert cls.__slots__ == () and not hasattr(cls(), "__dict__")


def test_abi_version_and_chunks(native):
    lib = native.lib()
    assert lib.cm_abi_version() == native.ABI_VERSION
    assert lib.cm_scan_num_chunks(1) == 1
    assert lib.cm_scan_num_chunks(64) == 1
    assert lib.cm_scan_num_chunks(65) == 2


def test_scan_chunk_policy_and_workspace_are_host_functions(native):
    """cm_scan_cl_fwd_auto_chunks / cm_scan_cl_fwd_workspace_bytes depend on sizes only (no GPU): large launches are not
    cut, launches of fewer than 256 workgroups are cut to ~1024 with chunks of at least 128 steps, and the workspace is
    three (ndir, batch, chunks, dim, 16) fp32 slabs for the chunk count the launch will really use."""
    lib = native.lib()
    auto = lib.cm_scan_cl_fwd_auto_chunks
    assert auto(64, 1000, 512, 2) == 1 and auto(16, 1000, 512, 2) == 1          # >= 256 workgroups
    assert auto(8, 1000, 512, 2) == 7                                           # 1024 // 128 = 8, capped at 1000 // 128
    assert auto(4, 4000, 1024, 2) == 8 and auto(1, 4000, 512, 2) == 31
    assert auto(1, 100, 64, 1) == 1 and auto(0, 100, 64, 1) == 1
    a = native.ScanClArgs()
    a.batch, a.seqlen, a.dim, a.ndir = 4, 4000, 1024, 2
    assert lib.cm_scan_cl_fwd_workspace_bytes(C.byref(a)) == 0                  # time_chunks 0 / 1: none
    a.time_chunks = 8                                                           # 4000 / 8 = 500 -> 512-step chunks -> 8 chunks
    assert lib.cm_scan_cl_fwd_workspace_bytes(C.byref(a)) == 3 * 2 * 4 * 8 * 1024 * 16 * 4
    a.seqlen, a.time_chunks = 50, 7                                             # 16-step chunks -> 4 chunks, not 7
    assert lib.cm_scan_cl_fwd_workspace_bytes(C.byref(a)) == 3 * 2 * 4 * 4 * 1024 * 16 * 4
    assert lib.cm_scan_cl_fwd_workspace_bytes(None) == 0
    # the backward's policy: under 512 workgroups (two per CU) it cuts to about 1024, chunks of at least 128 steps
    bauto = lib.cm_scan_cl_bwd_auto_chunks
    assert bauto(32, 1000, 512, 2) == 1 and bauto(64, 1000, 512, 2) == 1
    assert bauto(4, 4000, 1024, 2) == 8 and bauto(16, 1000, 512, 2) == 4 and bauto(1, 100, 64, 1) == 1
    b = native.ScanClBwdArgs()
    b.batch, b.seqlen, b.dim, b.ndir, b.time_chunks = 4, 4000, 1024, 2, 1
    b.dir[0].dt_rank = b.dir[1].dt_rank = 32
    one = lib.cm_scan_cl_bwd_workspace_bytes(C.byref(b))
    b.time_chunks = 0
    assert lib.cm_scan_cl_bwd_workspace_bytes(C.byref(b)) - one == 4 * 2 * 4 * 1024 * 7 * (16 + 32 + 4 + 3 * 16)


def test_bad_arguments_are_rejected_not_fatal(native):
    lib = native.lib()
    a = native.ScanFwdArgs()          # all zero: sizes invalid
    rc = lib.cm_selective_scan_fwd(C.byref(a))
    assert rc == -1
    assert b"bad sizes" in lib.cm_last_error()
    a.batch, a.dim, a.seqlen, a.dstate = 1, 8, 16, 16
    rc = lib.cm_selective_scan_fwd(C.byref(a))   # null pointers
    assert rc == -1 and b"non-NULL" in lib.cm_last_error()
    assert lib.cm_selective_scan_fwd(None) == -1
    c = native.ConvArgs()
    assert lib.cm_causal_conv1d_fwd(C.byref(c)) == -1
    b = native.ScanBwdArgs()
    assert lib.cm_selective_scan_bwd(C.byref(b)) == -1


def test_ops_refuse_cpu_tensors(native):
    import torch
    from mamba_asr_amd import ops
    x = torch.zeros(1, 8, 16)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.causal_conv1d_fwd(x, torch.zeros(8, 4))


def test_cast_cache_follows_in_place_updates(native):
    """ops.cast_cached (the bf16 weight copies the autograd nodes reuse within a step) must notice every in-place
    update of the parameter: optimizer steps, copy_ (load_state_dict) and updates through detach()."""
    import torch
    from mamba_asr_amd import ops
    p = torch.nn.Parameter(torch.randn(8, 8))
    c1 = ops.cast_cached(p, torch.bfloat16)
    assert ops.cast_cached(p, torch.bfloat16) is c1 and not c1.requires_grad
    opt = torch.optim.SGD([p], lr=0.5)
    p.grad = torch.ones_like(p)
    opt.step()
    c2 = ops.cast_cached(p, torch.bfloat16)
    assert c2 is not c1 and torch.equal(c2, p.detach().bfloat16())
    with torch.no_grad():
        p.copy_(torch.zeros(8, 8))
    assert torch.equal(ops.cast_cached(p, torch.bfloat16), torch.zeros(8, 8, dtype=torch.bfloat16))
    p.detach().add_(1.0)
    assert torch.equal(ops.cast_cached(p, torch.bfloat16), torch.ones(8, 8, dtype=torch.bfloat16))
    assert ops.cast_cached(p, torch.float32).data_ptr() == p.data_ptr()
