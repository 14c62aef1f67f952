"""CPU: the generated leaf chains (tools/gen_keccak_asm.py -> virgo-plus_amd/csrc/vp_keccak_asm.h) and the C / host surface of the masked fast path.
No compute call is made here."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

from conftest import ROOT

HEADER = os.path.join(ROOT, "virgo-plus_amd", "csrc", "vp_keccak_asm.h")
# SHA-256 of the text of vp_leaf_chain_asm (from its signature to its closing brace) in the header as it stood before vp_leaf_chain_mask_asm was generated beside it
UNMASKED_CHAIN_SHA256 = "f353455a8978f12c30a75098bc93cafac87454b2461cde857c2834b7301303dd"


def _function_text(src, name):
    a = src.index("__device__ __forceinline__ void %s(" % name)
    return src[a:src.index("}\n", a) + 2]


def test_generator_reproduces_the_header_and_leaves_the_unmasked_chain_alone():
    """The header is only ever written by the generator: its output is the committed file byte for byte; the unmasked chain's text is what it was before the
    masked chain was added (the unmasked kernels compile to what they were), and the masked chain — its rounds written as invocations of one assembler macro,
    expanded here by the assembler's rules — differs from it only in the block that closes the chain."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_keccak_asm.py")], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout
    committed = open(HEADER, "rb").read()
    assert out == committed
    src = committed.decode()
    plain = _function_text(src, "vp_leaf_chain_asm")
    assert hashlib.sha256(plain.encode()).hexdigest() == UNMASKED_CHAIN_SHA256
    masked = _function_text(src, "vp_leaf_chain_mask_asm")
    lines = lambda f: [l.strip()[1:-len('\\n\\t"')] for l in f.splitlines() if l.strip().startswith('"')]
    pl, ml = lines(plain), _expand(lines(masked))
    only_plain = [l for l in pl if l not in ml]
    only_masked = [l for l in ml if l not in pl]
    assert len(only_plain) == 8 and all(re.fullmatch(r"v_mov_b32 v\d+, 0", l) for l in only_plain)      # the zero fill of the eight message registers
    assert len(only_masked) == 4 and sum("global_load_dwordx4" in l for l in only_masked) == 2 and all("mask" in l or "s44" in l or "3f" in l for l in only_masked)
    assert len(pl) - len(ml) == 8 - 4                                             # eight zero moves out; a compare, a branch and two loads in
    assert "[mask0]" in masked and "[mask1]" in masked and "[mask0]" not in plain
    # both chains clobber the same fixed registers
    clob = lambda f: re.search(r': "memory".*\);', f).group(0)
    assert clob(plain) == clob(masked)


def _expand(ml):
    """what the assembler makes of the masked chain's text: .macro vp_kround lo, hi ... .endm in front, invocations replaced by the body with \\lo / \\hi filled
    in and the .if blocks of a zero argument dropped, .purgem behind"""
    assert ml[0] == ".macro vp_kround lo, hi" and ml[-1] == ".purgem vp_kround"
    end = ml.index(".endm")
    body, out = ml[1:end], []
    assert len(body) > 100 and sum(l.startswith("vp_kround ") for l in ml) >= 20
    for l in ml[end + 1:-1]:
        if not l.startswith("vp_kround "):
            out.append(l)
            continue
        arg = dict(zip(("lo", "hi"), l[len("vp_kround "):].split(", ")))
        keep = True
        for b in body:
            if b.startswith(".if "):
                keep = int(arg[b[len(".if ") + 2:]], 16) != 0
            elif b == ".endif":
                keep = True
            elif keep:
                out.append(b.replace("\\\\lo", arg["lo"]).replace("\\\\hi", arg["hi"]))
    return out


def _decl(header, name):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
    assert m, name
    return re.sub(r"\s+,", ",", re.sub(r"\s+", " ", m.group(1))).strip()


def test_new_symbols_are_declared_with_their_signatures_and_exported(vp):
    gpu_h = os.path.join(ROOT, "include", "vpgpu.h")
    host_h = os.path.join(ROOT, "virgo-plus_amd", "host", "vphost.h")
    assert _decl(gpu_h, "vp_commit_public_eq_masked") == ("vp_ctx *, const vp_F *point, int n_point, const vp_F *pub_mask, uint64_t n_pub_mask, vp_F *inner, "
                                                          "vp_F all_sum[65], uint8_t root_h[32]")
    assert _decl(host_h, "vph_commit_public_eq_masked") == ("vph_session *, const uint64_t *point_pairs, int n_point, const uint64_t *mask_pairs, uint64_t n_mask, "
                                                            "uint8_t out[32 + 16 + 65 * 16], double *ms, char *err, int errlen")
    assert _decl(host_h, "vph_prove_protocol_masked") == ("vph_session *, const uint64_t *pri_mask_pairs, uint64_t n_pri, const uint64_t *pub_mask_pairs, uint64_t n_pub, "
                                                          "uint8_t *transcript, uint64_t capacity, uint64_t *n_written, uint8_t *fri_roots, uint64_t roots_cap, "
                                                          "uint64_t *final_pairs, uint64_t *final_mask_pairs, double sec[6], int flags, char *err, int errlen")
    # the unmasked declarations stand as they were
    assert _decl(gpu_h, "vp_commit_public_eq") == "vp_ctx *, const vp_F *point, int n_point, vp_F *inner_product_sum, vp_F all_sum[65], uint8_t root_h[32]"
    assert _decl(gpu_h, "vp_pc_hash_late") == "vp_ctx *, int on" and "enum { VP_HASH_LATE_MASKED = 2 };" in open(gpu_h).read()
    assert "enum { VPH_PASS_DEFERRED = 1, VPH_PASS_QUEUE_NEXT = 2, VPH_PASS_HASH_PER_CALL = 4 };" in open(host_h).read()
    nm = lambda lib: subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert " T vp_commit_public_eq_masked" in nm(vp.LIB_GPU)
    host = nm(vp.LIB_HOST)
    assert " T vph_commit_public_eq_masked" in host and " T vph_prove_protocol_masked" in host
    for lib in (vp.LIB_GPU_CHECKED, vp.LIB_GPU_TESTDRV):
        if os.path.exists(lib):
            assert " T vp_commit_public_eq_masked" in nm(lib)
    # the Python layer binds them with the same argument counts
    assert len(vp.lib_gpu().vp_commit_public_eq_masked.argtypes) == 8
    assert len(vp.lib_host().vph_commit_public_eq_masked.argtypes) == 9 and len(vp.lib_host().vph_prove_protocol_masked.argtypes) == 16
    import inspect
    assert list(inspect.signature(vp.Session.prove_protocol).parameters)[1:] == ["deferred", "queue_next", "hash_per_call", "mask", "pub_mask"]
    assert list(inspect.signature(vp.Session.commit_public_eq).parameters)[1:] == ["point", "pub_mask"]


def test_masked_kernels_are_in_the_code_object_and_options_abi_is_unchanged(vp):
    """The leaf-hash family of the code object: the generated chain without and with the mask pair (the two instantiations of k_leaf_hash<MASK>, by their
    mangled template arguments) and the compiler's form — and none of the single-purpose copies they replaced."""
    data = open(vp.LIB_GPU, "rb").read()
    for k in (b"11k_leaf_hashILb0EE", b"11k_leaf_hashILb1EE", b"13k_leaf_hash_cE"):
        assert k in data, k
    for k in (b"k_leaf_hash_multi", b"k_leaf_hash_m", b"k_leaf_hash_cm", b"k_leaf_hash_final", b"k_merkle_level_multi", b"k_merkle_top_multi"):
        assert k not in data, k
    o = vp.Options()
    assert ctypes.sizeof(vp.Options) == 4 * (2 + 12 + 4) == o.struct_size
    hdr = open(os.path.join(ROOT, "include", "vpgpu.h")).read()
    assert int(re.search(r"#define VP_OPTIONS_ABI (0x[0-9a-f]+)u", hdr).group(1), 16) == vp.VP_OPTIONS_ABI
