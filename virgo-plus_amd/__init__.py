"""virgo-plus_amd — MI355X-native GKR sumcheck prover (Virgo++), Python harness side.

The product is native: ``csrc/`` (HIP kernels + the C ABI of include/vpgpu.h -> libvpgpu.so) and
``host/`` (C++ mirror of the reference's prover / verifier / circuit-loader API -> libvphost.so and the
``virgo_plus_run`` CLI).  This module only builds those in-tree and exposes them through ctypes for
tests/ and bench.py.  There is no CPU fallback: creating a Session without a working gfx950 device and
the built libraries raises.

The directory name contains a hyphen; load it with ``load()`` from the repo root's ``vp_loader.py`` or
importlib (see tests/conftest.py).
"""
import ctypes
import os
import shutil
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
HOST = os.path.join(PKG_DIR, "host")
# VP_LIBGPU: development override (A/B builds of the kernels under tools/_build/<variant>/libvpgpu.so are measured without touching the
# product library; build() never writes to an overridden path)
LIB_GPU = os.environ.get("VP_LIBGPU") or os.path.join(CSRC, "libvpgpu.so")
LIB_GPU_CHECKED = os.path.join(ROOT, "tools", "_build", "checked", "libvpgpu.so")      # -DVP_CHECKED flavour (csrc/vp_check.h), loaded through VP_LIBGPU by its test
LIB_GPU_TESTDRV = os.path.join(ROOT, "tools", "_build", "testdrv", "libvpgpu.so")      # -DVP_TEST_DRIVERS flavour: the launch plan's two cross-check drivers (VP_GKR_PATH=lanes|simple), loaded through VP_LIBGPU by their test
LIB_HOST = os.path.join(HOST, "libvphost.so")
CLI = os.path.join(HOST, "virgo_plus_run")

GPU_SRC = [os.path.join(CSRC, f) for f in ("vpgpu.hip", "vpgpu_batched.inc", "vpgpu_pc.inc", "vpgpu_pc_shard.inc", "vpgpu_pcverify.inc", "vp_kernels_pcverify.h", "vpgpu_fftgkr.inc", "vpgpu_gkrfs.inc", "vpgpu_upload.inc", "vp_kernels_fftgkr.h", "vp_kernels_gkrfs.h", "vp_kernels.h", "vp_kernels_round.h", "vp_kernels_persist.h", "vp_kernels_batch.h",
                                              "vp_kernels_plan.h", "vp_kernels_pc.h", "vp_kernels_ntt8.h", "vp_kernels_ntt_long.h", "vp_keccak_asm.h", "vp_check.h", "vp_field.h", "vp_fri_layout.h", "vp_pc_live.h", "vp_pc_corners.h")] + [
    os.path.join(ROOT, "include", "vpgpu.h")]
HOST_SRC = [os.path.join(HOST, f) for f in ("circuit.cpp", "prover.cpp", "verifier.cpp", "vphost.cpp")]
HOST_HDR = [os.path.join(HOST, f) for f in ("circuit.hpp", "prover.hpp", "verifier.hpp", "vphost.h", "field.hpp",
                                              "polynomial.hpp", "sha3.hpp", "pc_fs.hpp", "fft_gkr_fs.hpp", "gkr_fs.hpp", "fft_gkr_verify.hpp")]


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources if os.path.exists(s))


def _hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


def build(force=False, verbose=False):
    """Compile libvpgpu.so (hipcc, gfx950), libvphost.so and virgo_plus_run (g++) in-tree."""
    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    if os.environ.get("VP_LIBGPU"):
        pass                                            # development override: never rebuilt from here
    elif force or _stale(LIB_GPU, GPU_SRC):
        hipcc = _hipcc()
        if hipcc is None:
            if os.path.exists(LIB_GPU):
                return  # prebuilt library travelled with the tree (GPU box without a toolchain)
            raise RuntimeError("hipcc not found and no prebuilt libvpgpu.so")
        run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-value",
             "-o", LIB_GPU, os.path.join(CSRC, "vpgpu.hip")])
    if (force or _stale(LIB_GPU_CHECKED, GPU_SRC)) and _hipcc() is not None:
        os.makedirs(os.path.dirname(LIB_GPU_CHECKED), exist_ok=True)
        run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-value", "-DVP_CHECKED",
             "-o", LIB_GPU_CHECKED, os.path.join(CSRC, "vpgpu.hip")])
    if (force or _stale(LIB_GPU_TESTDRV, GPU_SRC)) and _hipcc() is not None:
        os.makedirs(os.path.dirname(LIB_GPU_TESTDRV), exist_ok=True)
        run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-value", "-DVP_TEST_DRIVERS",
             "-o", LIB_GPU_TESTDRV, os.path.join(CSRC, "vpgpu.hip")])
    if force or _stale(LIB_HOST, HOST_SRC + HOST_HDR + [LIB_GPU]):
        run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-pthread", "-o", LIB_HOST] + HOST_SRC +
            ["-L" + CSRC, "-lvpgpu", "-Wl,-rpath,$ORIGIN/../csrc", "-Wl,-rpath,/opt/rocm/lib"])
    if force or _stale(CLI, [os.path.join(HOST, "virgo_plus_run.cpp"), LIB_HOST]):
        run(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", "-o", CLI, os.path.join(HOST, "virgo_plus_run.cpp"),
             "-L" + HOST, "-lvphost", "-L" + CSRC, "-lvpgpu", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,$ORIGIN/../csrc",
             "-Wl,-rpath,/opt/rocm/lib"])


class VphResult(ctypes.Structure):
    _fields_ = [("prove_sec", ctypes.c_double), ("gkr_device_ms", ctypes.c_double), ("evaluate_ms", ctypes.c_double),
                ("verify_sec", ctypes.c_double), ("fold_ms", ctypes.c_double), ("fold_launches", ctypes.c_uint64),
                ("fold_bytes", ctypes.c_uint64), ("rounds", ctypes.c_uint64), ("launches", ctypes.c_uint64),
                ("proof_kb", ctypes.c_double), ("verified", ctypes.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RoundStat(ctypes.Structure):           # vp_round_stat (include/vpgpu.h)
    _fields_ = [("phase", ctypes.c_int32), ("layer", ctypes.c_int32), ("round", ctypes.c_int32), ("how", ctypes.c_int32), ("tables", ctypes.c_int32),
                ("bytes", ctypes.c_uint64), ("us", ctypes.c_double)]


class LaunchStat(ctypes.Structure):          # vp_launch_stat (include/vpgpu.h)
    _fields_ = [("kind", ctypes.c_int32), ("step", ctypes.c_int32), ("workgroups", ctypes.c_uint32), ("jobs", ctypes.c_uint32),
                ("rounds", ctypes.c_uint32), ("first_round", ctypes.c_uint32), ("bytes", ctypes.c_uint64), ("work", ctypes.c_uint64),
                ("us", ctypes.c_double)]


_gpu = None
_host = None


def lib_gpu():
    """ctypes handle of libvpgpu.so (raises if it is not built)."""
    global _gpu
    if _gpu is None:
        if not os.path.exists(LIB_GPU):
            raise RuntimeError("libvpgpu.so is not built: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_GPU, mode=ctypes.RTLD_GLOBAL)
        vp = ctypes.c_void_p
        L.vp_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        L.vp_create_with_options.argtypes = [ctypes.c_int, vp, ctypes.POINTER(vp)]
        L.vp_get_options.argtypes = [vp, vp]
        L.vp_get_resident_resumes.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
        L.vp_set_shard_split.argtypes = [vp, ctypes.c_int]
        L.vp_set_round_shard.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.vp_get_round_shard.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        L.vp_shard_finish.argtypes = [vp, vp, ctypes.c_uint64, vp]
        L.vp_gkr_sizes.argtypes = [vp, vp, vp]
        L.vp_options_default.argtypes = [vp]
        L.vp_tuning_get.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32)]
        u64_ = ctypes.c_uint64
        L.vp_set_deferred.argtypes = [vp, ctypes.c_int]
        L.vp_warm.argtypes = [vp, ctypes.c_uint32]
        L.vp_flush.argtypes = [vp, ctypes.c_int]
        L.vp_pending.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
        L.vp_pc_hash_late.argtypes = [vp, ctypes.c_int]
        L.vp_phase_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        L.vp_commit_private.argtypes = [vp, vp]
        L.vp_fft_gkr_sizes.argtypes = [ctypes.c_int, vp, vp]
        L.vp_fft_gkr.argtypes = [vp, ctypes.c_int, vp, u64_, vp, u64_, vp]
        L.vp_fft_gkr_begin.argtypes = [vp, ctypes.c_int, vp, u64_]
        L.vp_fft_gkr_end.argtypes = [vp, vp, u64_, vp]
        L.vp_fft_gkr_cancel.argtypes = [vp]
        L.vp_fft_gkr_fs.argtypes = [vp, ctypes.c_int, vp, vp, u64_, vp, vp, vp]
        L.vp_options_default.restype = None
        L.vp_destroy.argtypes = [vp]
        L.vp_last_error.argtypes = [vp]
        L.vp_last_error.restype = ctypes.c_char_p
        L.vp_version.restype = ctypes.c_char_p
        L.vp_test_field.argtypes = [vp, ctypes.c_int, vp, vp, vp, ctypes.c_uint64]
        L.vp_test_beta.argtypes = [vp, vp, ctypes.c_int, vp, vp]
        L.vp_test_sha3.argtypes = [vp, vp, vp, ctypes.c_uint64]
        L.vp_test_fft.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
        L.vp_pc_load_input.argtypes = [vp, vp, ctypes.c_uint64, ctypes.c_int]
        L.vp_pc_set_shard.argtypes = [vp, ctypes.c_int, ctypes.c_int]
        L.vp_shard_exchange_local.argtypes = [ctypes.POINTER(vp), ctypes.c_int]
        L.vp_commit_private.argtypes = [vp, vp]
        L.vp_commit_public.argtypes = [vp, vp, ctypes.c_uint64, vp, vp, vp]
        L.vp_commit_public_eq.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp]
        L.vp_commit_public_eq_masked.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_uint64, vp, vp, vp]
        L.vp_commit_public_masked.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp, vp]
        L.vp_fri_final_mask.argtypes = [vp, vp]
        L.vp_fri_commit.argtypes = [vp, vp, ctypes.c_int, vp]
        L.vp_fri_commit_fs.argtypes = [vp, vp, vp, vp, vp]
        L.vp_test_fs_draw.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_uint64, ctypes.c_uint64, vp, vp]
        L.vp_fs_grind.argtypes = [vp, vp, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), vp]
        L.vp_fri_step.argtypes = [vp, vp, vp]
        L.vp_commit_private_masked.argtypes = [vp, vp, ctypes.c_uint64, vp]
        L.vp_shard_pending.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
        L.vp_pc_shard_owner.argtypes = [vp, ctypes.c_int, ctypes.c_uint64]
        L.vp_fri_final.argtypes = [vp, vp]
        L.vp_fri_open.argtypes = [vp, ctypes.c_int, ctypes.c_uint64, vp, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.vp_fri_open_many.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int, vp]
        L.vp_fri_query_bytes.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
        L.vp_fri_query.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
        L.vp_pc_public_evals.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_int, vp, vp]
        L.vp_fri_query_digests.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_uint64, vp]
        L.vp_pc_mask_evals.argtypes = [vp, ctypes.c_int, vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, vp, vp]
        L.vp_commit_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        L.vp_comm_unique_id.argtypes = [vp]
        L.vp_comm_init.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int]
        L.vp_comm_destroy.argtypes = [vp]
        L.vp_comm_count.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
        L.vp_get_round_stats.argtypes = [vp, ctypes.POINTER(RoundStat), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.vp_allreduce_u64.argtypes = [vp, vp, ctypes.c_uint64]
        L.vp_set_profiling.argtypes = [vp, ctypes.c_int]
        L.vp_get_launch_stats.argtypes = [vp, ctypes.POINTER(LaunchStat), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.vp_kernel_name.argtypes = [ctypes.c_int]
        L.vp_get_gen_jobs.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
        L.vp_kernel_name.restype = ctypes.c_char_p
        _gpu = L
    return _gpu


def lib_host():
    """ctypes handle of libvphost.so (raises if it is not built)."""
    global _host
    if _host is None:
        lib_gpu()
        if not os.path.exists(LIB_HOST):
            raise RuntimeError("libvphost.so is not built: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_HOST)
        vp = ctypes.c_void_p
        u64 = ctypes.c_uint64
        L.vph_circuit_from_pws.restype = vp
        L.vph_circuit_from_pws.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_long, ctypes.c_char_p, ctypes.c_int]
        L.vph_circuit_randomize.restype = vp
        L.vph_circuit_randomize.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_long]
        L.vph_circuit_custom.restype = vp
        L.vph_circuit_custom.argtypes = [ctypes.c_int] + [vp] * 7
        L.vph_circuit_free.argtypes = [vp]
        L.vph_circuit_layers.argtypes = [vp]
        L.vph_circuit_gates.restype = u64
        L.vph_circuit_gates.argtypes = [vp]
        L.vph_circuit_layer_size.restype = u64
        L.vph_circuit_layer_size.argtypes = [vp, ctypes.c_int]
        L.vph_circuit_layer_bitlen.argtypes = [vp, ctypes.c_int]
        L.vph_circuit_hash.argtypes = [vp, ctypes.POINTER(u64)]
        L.vph_session_create.restype = vp
        L.vph_session_create.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.vph_session_create_opts.restype = vp
        L.vph_session_create_opts.argtypes = [vp, ctypes.c_int, vp, ctypes.c_char_p, ctypes.c_int]
        L.vph_session_create_round_sharded.restype = vp
        L.vph_session_create_round_sharded.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, vp, ctypes.c_char_p, ctypes.c_int]
        L.vph_session_create_sharded.restype = vp
        L.vph_session_create_sharded.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_char_p, ctypes.c_int]
        L.vph_commit_private_masked.argtypes = [vp, vp, u64, vp, ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ctypes.c_int]
        L.vph_commit_public_eq.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ctypes.c_int]
        L.vph_commit_public_eq_masked.argtypes = [vp, vp, ctypes.c_int, vp, u64, vp, ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ctypes.c_int]
        L.vph_fri_open_many.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int, vp, ctypes.c_char_p, ctypes.c_int]
        L.vph_fri_query.argtypes = [vp, ctypes.c_int, vp, vp, u64, ctypes.POINTER(u64), ctypes.c_char_p, ctypes.c_int]
        L.vph_session_rank_ctx.restype = vp
        L.vph_session_rank_ctx.argtypes = [vp, ctypes.c_int]
        L.vph_session_world.argtypes = [vp]
        L.vph_session_partials.argtypes = [vp, vp, ctypes.c_int]
        L.vph_session_clear_partials.argtypes = [vp]
        L.vph_session_drop_rank.argtypes = [vp, ctypes.c_int]
        L.vph_session_gather_sec.restype = ctypes.c_double
        L.vph_session_gather_sec.argtypes = [vp]
        L.vph_session_free.argtypes = [vp]
        L.vph_set_profiling.argtypes = [vp, ctypes.c_int]
        L.vph_session_ctx.restype = vp
        L.vph_session_ctx.argtypes = [vp]
        L.vph_layer_values.argtypes = [vp, ctypes.c_int, vp, u64]
        L.vph_prove_interactive.argtypes = [vp, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(VphResult), ctypes.c_char_p,
                                            ctypes.c_int]
        L.vph_draw_tape.argtypes = [vp]
        L.vph_set_tape.argtypes = [vp, vp, u64]
        L.vph_verify_transcript_tape.argtypes = [vp, vp, u64, vp, u64, ctypes.c_int]
        L.vph_prove_gkr.argtypes = [vp, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(VphResult), ctypes.c_char_p, ctypes.c_int]
        L.vph_check.argtypes = [vp, vp, u64, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
        L.vph_verify_transcript.argtypes = [vp, vp, u64, ctypes.c_int]
        L.vph_commit_public.argtypes = [vp, vp, u64, vp, ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ctypes.c_int]
        L.vph_prove_full.argtypes = [vp, vp, u64, ctypes.POINTER(u64), ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.vph_prove_and_verify_full.argtypes = [vp, ctypes.c_int, vp, u64, ctypes.POINTER(u64)] + [ctypes.POINTER(ctypes.c_double)] * 3 + [ctypes.c_char_p, ctypes.c_int]
        L.vph_prove_and_verify_full_ex.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, u64, ctypes.POINTER(u64)] + [ctypes.POINTER(ctypes.c_double)] * 3 + [ctypes.c_char_p, ctypes.c_int]
        L.vph_prove_and_verify_full_masked.argtypes = ([vp, ctypes.c_int, ctypes.c_int, vp, u64, vp, u64, vp, u64, ctypes.POINTER(u64)] + [ctypes.POINTER(ctypes.c_double)] * 3 +
                                                       [ctypes.c_char_p, ctypes.c_int])
        L.vph_pc_mask_evals_host.argtypes = [ctypes.c_int, vp, u64, u64, ctypes.c_int, vp, vp]
        L.vph_pc_mask_evals.argtypes = [vp, ctypes.c_int, vp, u64, u64, ctypes.c_int, vp, vp, ctypes.c_char_p, ctypes.c_int]
        L.vph_verify_commitment.argtypes = [ctypes.c_int, vp, vp, vp, u64, u64] + [vp] * 8 + [ctypes.c_int, vp, vp, u64, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.vph_commit_fs.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, u64, vp, u64, ctypes.c_int, vp, u64, ctypes.POINTER(u64), ctypes.c_char_p, ctypes.c_int]
        L.vph_last_commit_fs_times.restype = None
        L.vph_last_commit_fs_times.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        L.vph_verify_commitment_fs.argtypes = [vp, u64, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.vph_commitment_fs_challenges.argtypes = [vp, u64, vp, vp]
        L.vph_prove_full_fs.argtypes = [vp, ctypes.c_int, vp, u64, vp, u64, vp, u64, ctypes.POINTER(u64), vp, ctypes.c_char_p, ctypes.c_int]
        L.vph_verify_full_fs.argtypes = [vp, vp, u64, ctypes.c_int, vp, ctypes.c_char_p, ctypes.c_int]
        L.vph_prove_full_fs_ex.argtypes = [vp, ctypes.c_int, vp, u64, vp, u64, vp, u64, ctypes.POINTER(u64), vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.vph_fs_grind_host.argtypes = [vp, ctypes.c_int, u64, u64, ctypes.POINTER(u64), vp]
        L.vph_commit_fs_pow.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, u64, vp, u64, ctypes.c_int, ctypes.c_int, vp, u64, ctypes.POINTER(u64), ctypes.c_char_p, ctypes.c_int]
        L.vph_verify_commitment_fs_min.argtypes = [vp, u64, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.vph_fs_pow.argtypes = [vp, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]
        L.vph_prove_full_fs_pow.argtypes = [vp, ctypes.c_int, vp, u64, vp, u64, vp, u64, ctypes.POINTER(u64), vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.vph_verify_full_fs_min.argtypes = [vp, vp, u64, ctypes.c_int, ctypes.c_int, vp, ctypes.c_char_p, ctypes.c_int]
        L.vph_prove_fs_ex.argtypes = [vp, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(VphResult), ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.vph_gkr_sizes.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
        L.vph_gkr_fs_tape.argtypes = [vp, vp, vp, u64, vp, ctypes.POINTER(u64), vp]
        L.vph_prove_gkr_fs.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64), vp, ctypes.POINTER(u64), vp, ctypes.c_char_p, ctypes.c_int]
        L.vph_fft_gkr_fs_tape.argtypes = [ctypes.c_int, vp, vp, u64, vp, vp]
        L.vph_fft_gkr_check.argtypes = [ctypes.c_int, vp, u64, vp, u64]
        L.vph_fft_gkr_fs.argtypes = [vp, ctypes.c_int, vp, vp, u64, vp, vp, ctypes.c_char_p, ctypes.c_int]
        L.vph_last_full_record.argtypes = [vp, vp, u64, ctypes.POINTER(u64)]
        L.vph_verify_full_record.argtypes = [vp, vp, u64]
        L.vph_verifier_launches.argtypes = [vp, ctypes.POINTER(LaunchStat), ctypes.c_int]
        L.vph_verify_full_record_dev.argtypes = [vp, ctypes.c_int, vp, u64, ctypes.c_char_p, ctypes.c_int]
        L.vph_last_verify_split.restype = None
        L.vph_last_verify_split.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        L.vph_pc_public_evals_host.argtypes = [ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int, vp, vp]
        L.vph_pc_opening_digests_host.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, u64, vp]
        L.vph_pc_query_answer_bytes.restype = u64
        L.vph_pc_query_answer_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
        L.vph_pc_public_evals.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_int, vp, vp, ctypes.c_char_p, ctypes.c_int]
        L.vph_fri_query_digests.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, u64, vp, ctypes.c_char_p, ctypes.c_int]
        L.vph_last_fri.argtypes = [vp, vp, u64, vp, vp]
        L.vph_draw_protocol_tape.argtypes = [vp]
        L.vph_prove_protocol.argtypes = [vp, vp, u64, ctypes.POINTER(u64), vp, u64, vp, ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ctypes.c_int]
        L.vph_prove_protocol_ex.argtypes = [vp, vp, u64, ctypes.POINTER(u64), vp, u64, vp, ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.vph_prove_protocol_masked.argtypes = [vp, vp, u64, vp, u64, vp, u64, ctypes.POINTER(u64), vp, u64, vp, vp, ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.vph_last_point.argtypes = [vp, vp, ctypes.c_int]
        L.vph_last_fft_gkr.restype = ctypes.c_int64
        L.vph_last_fft_gkr.argtypes = [vp, vp, u64]
        L.vph_last_pc_times.restype = None
        L.vph_last_pc_times.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        L.vph_interactive_breakdown.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        L.vph_test_sha3.argtypes = [vp, vp, u64]
        L.vph_fri_commit.argtypes = [vp, vp, ctypes.c_int, vp, vp, ctypes.c_char_p, ctypes.c_int]
        L.vph_fri_commit_batched.argtypes = [vp, vp, ctypes.c_int, vp, vp, ctypes.c_char_p, ctypes.c_int]
        L.vph_commit_private.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ctypes.c_int]
        L.vph_prove_fs.argtypes = [vp, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(VphResult), ctypes.c_char_p, ctypes.c_int]
        L.vph_verify_fs.argtypes = [vp, vp, u64]
        L.vph_last_gkr_failure.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        L.vph_commit_device_ms.restype = ctypes.c_double
        L.vph_commit_device_ms.argtypes = [vp]
        L.vph_set_shard.argtypes = [vp, ctypes.c_int, ctypes.c_int]
        L.vph_shard_chains.argtypes = [vp, vp, vp, ctypes.c_int]
        L.vph_shard_vu_partials.argtypes = [vp, vp, ctypes.c_int]
        L.vph_shard_vu_set.argtypes = [vp, vp, ctypes.c_int]
        L.vph_transcript_bytes.restype = u64
        L.vph_transcript_bytes.argtypes = [vp]
        _host = L
    return _host


GKR_CHECKS = (None, "phase1", "phase2", "semi_final", "liu", "liu_semi_final", "input")


def _fs_grind_args(state, bits, first, max_tries):
    state, bits, first = bytes(state), int(bits), int(first)
    if len(state) != 32:
        raise ValueError("fs_grind: a 32-byte state")
    if max_tries is None:                                      # 64 x 2^bits tries, as the provers search, cut at 2^64
        max_tries = min(64 << max(bits, 0), (1 << 64) - first) if 0 <= first < 1 << 64 else 0
    max_tries = int(max_tries)
    if not (1 <= bits <= 48 and 0 <= first < 1 << 64 and 1 <= max_tries and first + max_tries <= 1 << 64):
        raise ValueError("fs_grind: bits in 1..48 and a non-empty range [first, first + max_tries) within 2^64")
    return state, bits, first, max_tries


def fs_grind_host(state, bits, first=0, max_tries=None):
    """The proof-of-work search on the CPU (vph_fs_grind_host, host/vphost.h): the smallest nonce in [first, first + max_tries) whose chain step
    W(bits, nonce) on the 32-byte `state` leaves the low `bits` bits of the new state's first word zero.  Returns (nonce, state_out); raises ValueError on
    arguments outside the limits and RuntimeError when the range holds no such nonce.  max_tries None: 64 x 2^bits."""
    state, bits, first, max_tries = _fs_grind_args(state, bits, first, max_tries)
    st_in, st_out, nonce = ctypes.create_string_buffer(state, 32), ctypes.create_string_buffer(32), ctypes.c_uint64(0)
    rc = lib_host().vph_fs_grind_host(ctypes.cast(st_in, ctypes.c_void_p), bits, first, max_tries, ctypes.byref(nonce), ctypes.cast(st_out, ctypes.c_void_p))
    if rc == -5:
        raise RuntimeError("fs_grind_host: no nonce in the range meets the work")
    if rc:
        raise ValueError("fs_grind_host: refused")
    return int(nonce.value), st_out.raw


def last_gkr_failure():
    """The first failed check of this thread's last GKR replay (vph_last_gkr_failure, host/vphost.h): None, or (kind, layer, round) with kind one of GKR_CHECKS and
    round -1 for a closing check.  Set by Circuit.verify_transcript(_tape), verify_fs, verify_full_record, verify_full_fs and Session.check."""
    layer, rnd = ctypes.c_int(0), ctypes.c_int(-1)
    kind = lib_host().vph_last_gkr_failure(ctypes.byref(layer), ctypes.byref(rnd))
    return (GKR_CHECKS[kind], layer.value, rnd.value) if kind else None


def sum_transcripts(parts):
    """Element-wise u64 sum (mod 2^64) of the transcripts of a sharded proof = what the all-reduce over RCCL computes.  The
    ranks' slices are disjoint and everything else is zero, so the sum is the unsharded transcript."""
    import numpy as np
    acc = np.zeros(len(parts[0]) // 8, dtype=np.uint64)
    for p in parts:
        acc += np.frombuffer(p, dtype=np.uint64)
    return acc.tobytes()


def allreduce_transcript(tr, device=None):
    """The one data-path collective of a sharded proof: all-reduce (sum, int64 lanes) of the transcript over the default
    torch.distributed group — RCCL over xGMI when the group's backend is "nccl" (the transcript goes through a device tensor),
    gloo on the CPU in the tests.  Returns the assembled transcript bytes on every rank."""
    import numpy as np
    import torch
    import torch.distributed as dist
    t = torch.from_numpy(np.frombuffer(tr, dtype=np.int64).copy())
    if "nccl" in dist.get_backend():
        t = t.cuda(device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu().numpy().tobytes()


OPEN_PATH_STRIDE = 32 * 26      # bytes per request that fri_open_many reserves for a path (the longest one, at an input layer of 2^25 wires, is 24 digests)


def fri_open_many(ctx, requests, path_stride=OPEN_PATH_STRIDE, fill=0):
    """vp_fri_open_many on a vp_ctx*: requests = sequence of (oracle, leaf).  Returns (rc, values (n, 130, 2) uint64, paths (n, path_stride) uint8,
    path_len (n,) int32); the output arrays are pre-filled with the byte `fill`, so that what the library left untouched can be told."""
    import numpy as np
    n = len(requests)
    oracle = np.ascontiguousarray([r[0] for r in requests], dtype=np.int32).reshape(n)
    leaf = np.ascontiguousarray([r[1] for r in requests], dtype=np.uint64).reshape(n)
    values = np.full(max(n, 1) * 130 * 16, fill, dtype=np.uint8).view(np.uint64).reshape(-1, 130, 2)
    paths = np.full((max(n, 1), max(path_stride, 1)), fill, dtype=np.uint8)
    path_len = np.full(max(n, 1) * 4, fill, dtype=np.uint8).view(np.int32)
    rc = lib_gpu().vp_fri_open_many(ctx, n, oracle.ctypes.data, leaf.ctypes.data, values.ctypes.data, paths.ctypes.data, path_stride, path_len.ctypes.data)
    return rc, values[:n], paths[:n], path_len[:n]


def fri_query_bytes(ctx, n_queries):
    """(rc, size in bytes of vp_fri_query's answer to n_queries repetitions)."""
    b = ctypes.c_uint64(0)
    rc = lib_gpu().vp_fri_query_bytes(ctx, n_queries, ctypes.byref(b))
    return rc, b.value


def fri_query(ctx, leaf0):
    """vp_fri_query on a vp_ctx*: (rc, bytes).  leaf0[q] = the leaf of the two first oracles of repetition q."""
    import numpy as np
    leaf0 = np.ascontiguousarray(leaf0, dtype=np.uint64)
    rc, cap = fri_query_bytes(ctx, leaf0.shape[0])
    if rc:
        return rc, b""
    out = ctypes.create_string_buffer(max(cap, 1))
    n = ctypes.c_uint64(0)
    rc = lib_gpu().vp_fri_query(ctx, leaf0.shape[0], leaf0.ctypes.data, ctypes.cast(out, ctypes.c_void_p), cap, ctypes.byref(n))
    return rc, out.raw[: n.value] if rc == 0 else b""


class ShardedCommitment:
    """The Virgo commitment sharded over `world` ranks (include/vpgpu.h: vp_pc_set_shard), rehearsed as `world` light contexts of ONE
    process on one GPU: every rank runs the same entry points a multi-GPU run would, the collectives between them (one all-to-all per
    committed oracle, one all-gather of the level-5 tree nodes) are performed by vp_shard_exchange_local instead of RCCL."""
    VP_EXCHANGE = 1

    def __init__(self, inputs, bit_length, world, device=0):
        import numpy as np
        L = lib_gpu()
        self.world, self.n = world, bit_length
        inputs = np.ascontiguousarray(inputs, dtype=np.uint64)
        self.ctx = []
        for r in range(world):
            c = ctypes.c_void_p()
            if L.vp_create(device, ctypes.byref(c)):
                raise RuntimeError("vp_create failed")
            self.ctx.append(c)
            self._chk(L.vp_pc_load_input(c, inputs.ctypes.data, inputs.shape[0], bit_length), c, "vp_pc_load_input")
            self._chk(L.vp_pc_set_shard(c, r, world), c, "vp_pc_set_shard")
        self.arr = (ctypes.c_void_p * world)(*[c.value for c in self.ctx])

    @staticmethod
    def _chk(rc, c, what):
        if rc < 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, lib_gpu().vp_last_error(c).decode()))

    def _run(self, call, what):
        """call(rank) on every rank until all report VP_OK, exchanging whenever all report VP_EXCHANGE."""
        L = lib_gpu()
        for _ in range(8):
            rcs = [call(r) for r in range(self.world)]
            for r, rc in enumerate(rcs):
                self._chk(rc, self.ctx[r], what)
            if all(rc == 0 for rc in rcs):
                return
            if not all(rc == self.VP_EXCHANGE for rc in rcs):
                raise RuntimeError("%s: ranks disagree on the protocol stage %r" % (what, rcs))
            self._chk(L.vp_shard_exchange_local(self.arr, self.world), self.ctx[0], "vp_shard_exchange_local")
        raise RuntimeError("%s did not finish" % what)

    def device_ms(self):
        out = []
        for c in self.ctx:
            ms = ctypes.c_double(0)
            lib_gpu().vp_commit_stats(c, ctypes.byref(ms))
            out.append(ms.value)
        return out

    def commit_private(self):
        roots = [ctypes.create_string_buffer(32) for _ in range(self.world)]
        self._run(lambda r: lib_gpu().vp_commit_private(self.ctx[r], ctypes.cast(roots[r], ctypes.c_void_p)), "vp_commit_private")
        assert all(x.raw == roots[0].raw for x in roots), "ranks disagree on the root"
        return roots[0].raw

    def commit_public(self, pub):
        import numpy as np
        pub = np.ascontiguousarray(pub, dtype=np.uint64)
        roots = [ctypes.create_string_buffer(32) for _ in range(self.world)]
        inner = [np.zeros(2, np.uint64) for _ in range(self.world)]
        alls = [np.zeros((65, 2), np.uint64) for _ in range(self.world)]
        self._run(lambda r: lib_gpu().vp_commit_public(self.ctx[r], pub.ctypes.data, pub.shape[0], inner[r].ctypes.data, alls[r].ctypes.data,
                                                       ctypes.cast(roots[r], ctypes.c_void_p)), "vp_commit_public")
        for r in range(1, self.world):
            assert roots[r].raw == roots[0].raw and inner[r].tobytes() == inner[0].tobytes() and alls[r].tobytes() == alls[0].tobytes()
        return roots[0].raw, inner[0].tobytes(), alls[0].tobytes()

    def fri_commit(self, r):
        import numpy as np
        r = np.ascontiguousarray(r, dtype=np.uint64)
        st = r.shape[0]
        roots = [ctypes.create_string_buffer(32 * st) for _ in range(self.world)]
        self._run(lambda k: lib_gpu().vp_fri_commit(self.ctx[k], r.ctypes.data, st, ctypes.cast(roots[k], ctypes.c_void_p)), "vp_fri_commit")
        fins = []
        for k in range(self.world):
            fin = np.zeros((2048, 2), dtype=np.uint64)
            self._chk(lib_gpu().vp_fri_final(self.ctx[k], fin.ctypes.data), self.ctx[k], "vp_fri_final")
            fins.append(fin)
        for k in range(1, self.world):
            assert roots[k].raw == roots[0].raw and np.array_equal(fins[k], fins[0])
        return roots[0].raw, fins[0]

    def open(self, oracle, leaf, rank=None):
        """(values (130, 2), path digests) of one leaf, asked of its owner (or of `rank`)."""
        import numpy as np
        owner = ((leaf >> 5) % self.world) if rank is None else rank
        vals = np.zeros((130, 2), dtype=np.uint64)
        path = ctypes.create_string_buffer(32 * 40)
        n = ctypes.c_int(0)
        rc = lib_gpu().vp_fri_open(self.ctx[owner], oracle, leaf, vals.ctypes.data, ctypes.cast(path, ctypes.c_void_p), len(path), ctypes.byref(n))
        if rc:
            return None
        return vals, [path.raw[32 * i:32 * i + 32] for i in range(n.value)]

    def open_many(self, requests, path_stride=OPEN_PATH_STRIDE):
        """vp_fri_open_many asked of EVERY rank and merged by path_len (a rank reports 0 for a request it does not own and leaves its bytes alone).
        Returns (values (n, 130, 2), paths (n, path_stride) uint8, path_len (n,), answered (world, n) bool: which rank answered which request)."""
        import numpy as np
        n = len(requests)
        values = np.zeros((n, 130, 2), dtype=np.uint64)
        paths = np.zeros((n, path_stride), dtype=np.uint8)
        path_len = np.zeros(n, dtype=np.int32)
        answered = np.zeros((self.world, n), dtype=bool)
        for r in range(self.world):
            rc, v, p, pl = fri_open_many(self.ctx[r], requests, path_stride)
            self._chk(-abs(rc) if rc else 0, self.ctx[r], "vp_fri_open_many")
            mine = pl > 0
            answered[r] = mine
            values[mine], paths[mine], path_len[mine] = v[mine], p[mine], pl[mine]
        return values, paths, path_len, answered

    def close(self):
        for c in self.ctx:
            lib_gpu().vp_destroy(c)
        self.ctx = []


class ShardedCommitmentRank:
    """ONE rank of the Virgo commitment sharded over the ranks of a torch.distributed job (include/vpgpu.h: vp_pc_set_shard): a light
    context holding the input layer.  transport="rccl": the collectives (one all-to-all per committed oracle, one all-gather of tree nodes)
    run inside the entry points over an RCCL communicator attached to the context (needs one GPU per rank).  transport="host": no
    communicator — every call that returns VP_EXCHANGE has its pending collectives moved by torch.distributed on host buffers (gloo; the
    all-to-all as an all-gather of every rank's send side), which is how more ranks than GPUs are rehearsed and how the CPU suite's
    world-size-2 test drives it."""
    VP_EXCHANGE = 1

    def __init__(self, inputs, bit_length, rank, world, device=0, transport="rccl"):
        import numpy as np
        L = lib_gpu()
        for f in ("vp_shard_pending", "vp_shard_exchange_done"):
            getattr(L, f).argtypes = [ctypes.c_void_p] + ([ctypes.POINTER(ctypes.c_int)] if f == "vp_shard_pending" else [])
        L.vp_shard_exchange_info.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)]
        L.vp_shard_exchange_get.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.vp_shard_exchange_put.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        self.rank, self.world, self.n, self.transport = rank, world, bit_length, transport
        inputs = np.ascontiguousarray(inputs, dtype=np.uint64)
        self.ctx = ctypes.c_void_p()
        if L.vp_create(device, ctypes.byref(self.ctx)):
            raise RuntimeError("vp_create failed")
        self._chk(L.vp_pc_load_input(self.ctx, inputs.ctypes.data, inputs.shape[0], bit_length), "vp_pc_load_input")
        if transport == "rccl":
            import torch
            import torch.distributed as dist
            uid = ctypes.create_string_buffer(128)
            if rank == 0 and L.vp_comm_unique_id(ctypes.cast(uid, ctypes.c_void_p)):
                raise RuntimeError("vp_comm_unique_id failed (librccl.so.1 not found?)")
            t = torch.from_numpy(np.frombuffer(uid.raw, dtype=np.uint8).copy())
            if "nccl" in dist.get_backend():
                t = t.cuda()
            dist.broadcast(t, src=0)
            idb = ctypes.create_string_buffer(t.cpu().numpy().tobytes(), 128)
            self._chk(L.vp_comm_init(self.ctx, ctypes.cast(idb, ctypes.c_void_p), rank, world), "vp_comm_init")
        self._chk(L.vp_pc_set_shard(self.ctx, rank, world), "vp_pc_set_shard")

    def _chk(self, rc, what):
        if rc < 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, lib_gpu().vp_last_error(self.ctx).decode()))

    def comm_count(self):
        n = ctypes.c_int(0)
        self._chk(lib_gpu().vp_comm_count(self.ctx, ctypes.byref(n)), "vp_comm_count")
        return n.value

    def _exchange_host(self):
        import numpy as np
        import torch
        import torch.distributed as dist
        L = lib_gpu()
        n = ctypes.c_int(0)
        L.vp_shard_pending(self.ctx, ctypes.byref(n))
        for i in range(n.value):
            kind, nb = ctypes.c_int(0), ctypes.c_uint64(0)
            self._chk(L.vp_shard_exchange_info(self.ctx, i, ctypes.byref(kind), ctypes.byref(nb)), "vp_shard_exchange_info")
            b = int(nb.value)
            send = np.zeros(self.world * b if kind.value == 1 else b, dtype=np.uint8)
            self._chk(L.vp_shard_exchange_get(self.ctx, i, send.ctypes.data), "vp_shard_exchange_get")
            parts = [torch.zeros(send.shape[0], dtype=torch.uint8) for _ in range(self.world)]
            dist.all_gather(parts, torch.from_numpy(send))
            if kind.value == 1:        # all-to-all: from every peer p, the block it addressed to this rank
                recv = np.concatenate([parts[p].numpy()[self.rank * b:(self.rank + 1) * b] for p in range(self.world)])
            else:
                recv = np.concatenate([parts[p].numpy() for p in range(self.world)])
            recv = np.ascontiguousarray(recv)
            self._chk(L.vp_shard_exchange_put(self.ctx, i, recv.ctypes.data), "vp_shard_exchange_put")
        L.vp_shard_exchange_done(self.ctx)

    def _run(self, call, what):
        for _ in range(8):
            rc = call()
            self._chk(rc, what)
            if rc == 0:
                return
            if rc != self.VP_EXCHANGE or self.transport != "host":
                raise RuntimeError("%s: unexpected return %d" % (what, rc))
            self._exchange_host()
        raise RuntimeError("%s did not finish" % what)

    def device_ms(self):
        ms = ctypes.c_double(0)
        lib_gpu().vp_commit_stats(self.ctx, ctypes.byref(ms))
        return ms.value

    def commit_private(self):
        root = ctypes.create_string_buffer(32)
        self._run(lambda: lib_gpu().vp_commit_private(self.ctx, ctypes.cast(root, ctypes.c_void_p)), "vp_commit_private")
        return root.raw

    def commit_public(self, pub):
        import numpy as np
        pub = np.ascontiguousarray(pub, dtype=np.uint64)
        root = ctypes.create_string_buffer(32)
        inner, alls = np.zeros(2, np.uint64), np.zeros((65, 2), np.uint64)
        self._run(lambda: lib_gpu().vp_commit_public(self.ctx, pub.ctypes.data, pub.shape[0], inner.ctypes.data, alls.ctypes.data,
                                                     ctypes.cast(root, ctypes.c_void_p)), "vp_commit_public")
        return root.raw, inner.tobytes(), alls.tobytes()

    def fri_commit(self, r):
        import numpy as np
        r = np.ascontiguousarray(r, dtype=np.uint64)
        roots = ctypes.create_string_buffer(32 * r.shape[0])
        self._run(lambda: lib_gpu().vp_fri_commit(self.ctx, r.ctypes.data, r.shape[0], ctypes.cast(roots, ctypes.c_void_p)), "vp_fri_commit")
        fin = np.zeros((2048, 2), dtype=np.uint64)
        self._chk(lib_gpu().vp_fri_final(self.ctx, fin.ctypes.data), "vp_fri_final")
        return roots.raw, fin

    def close(self):
        if self.ctx:
            lib_gpu().vp_destroy(self.ctx)
            self.ctx = None


class Circuit:
    """layeredCircuit after subsetInit (host/circuit.hpp)."""

    def __init__(self, handle):
        if not handle:
            raise RuntimeError("circuit construction failed")
        self.h = handle

    @classmethod
    def from_pws(cls, path, blocks=1, seed=-1):
        err = ctypes.create_string_buffer(256)
        h = lib_host().vph_circuit_from_pws(os.fsencode(path), blocks, seed, err, len(err))
        if not h:
            raise RuntimeError("from_pws: " + err.value.decode())
        return cls(h)

    @classmethod
    def randomize(cls, layers, log_size, seed=-1):
        return cls(lib_host().vph_circuit_randomize(layers, log_size, seed))

    @classmethod
    def custom(cls, layer_sizes, ty, l, u, v, c_pairs, is_assert):
        """Arbitrary layered circuit from flat numpy arrays (see vphost.h)."""
        import numpy as np
        a = [np.ascontiguousarray(layer_sizes, np.uint64), np.ascontiguousarray(ty, np.int32), np.ascontiguousarray(l, np.int32),
             np.ascontiguousarray(u, np.uint64), np.ascontiguousarray(v, np.uint64), np.ascontiguousarray(c_pairs, np.uint64),
             np.ascontiguousarray(is_assert, np.uint8)]
        return cls(lib_host().vph_circuit_custom(len(a[0]), *[x.ctypes.data for x in a]))

    @property
    def layers(self):
        return lib_host().vph_circuit_layers(self.h)

    @property
    def gates(self):
        return lib_host().vph_circuit_gates(self.h)

    def layer_size(self, i):
        return lib_host().vph_circuit_layer_size(self.h, i)

    def layer_bitlen(self, i):
        return lib_host().vph_circuit_layer_bitlen(self.h, i)

    def hash(self):
        out = (ctypes.c_uint64 * 2)()
        lib_host().vph_circuit_hash(self.h, out)
        return "%016x%016x" % (out[0], out[1])

    def verify_transcript(self, transcript, skip_predicates=False):
        """Host verifier replay (no GPU): F::init(), draw the tape, check the GKR transcript."""
        buf = ctypes.create_string_buffer(bytes(transcript), len(transcript))
        return lib_host().vph_verify_transcript(self.h, ctypes.cast(buf, ctypes.c_void_p), len(transcript),
                                                1 if skip_predicates else 0) == 0

    def verify_transcript_tape(self, tape, transcript, skip_predicates=False):
        """Host verifier replay (no GPU) of a GKR transcript against the caller's tape, an (n, 2) uint64 array in draw order.  Raises when the tape does
        not fit the circuit (length, a limb >= p)."""
        import numpy as np
        t = np.ascontiguousarray(tape, dtype=np.uint64).reshape(-1, 2)
        buf = ctypes.create_string_buffer(bytes(transcript), max(len(transcript), 1))
        rc = lib_host().vph_verify_transcript_tape(self.h, t.ctypes.data, int(t.shape[0]), ctypes.cast(buf, ctypes.c_void_p), len(transcript),
                                                   1 if skip_predicates else 0)
        if rc < 0:
            raise ValueError("verify_transcript_tape: the tape does not fit the circuit")
        return rc == 0

    def verify_full_record(self, record, device=None):
        """Verify the record of a complete-protocol run (Session.last_full_record) on the host: no GPU, no session.  device=k: the same replay with the
        verifier's heavy loops (wiring predicates, public polynomial values, opening digests) on GPU k, on a context made for the call; the comparisons
        and the verdict stay on the host."""
        buf = ctypes.create_string_buffer(bytes(record), max(len(record), 1))
        if device is not None:
            err = ctypes.create_string_buffer(512)
            rc = lib_host().vph_verify_full_record_dev(self.h, int(device), ctypes.cast(buf, ctypes.c_void_p), len(record), err, len(err))
            if rc < 0:
                raise RuntimeError("verify_full_record(device=%d) failed: %s" % (device, err.value.decode()))
            return rc == 0
        return lib_host().vph_verify_full_record(self.h, ctypes.cast(buf, ctypes.c_void_p), len(record)) == 0

    @staticmethod
    def pc_query_answer_bytes(n, n_queries):
        """Size of vp_fri_query's answer to n_queries positions at input bit length n."""
        return int(lib_host().vph_pc_query_answer_bytes(int(n), int(n_queries)))

    @staticmethod
    def pc_public_evals_host(n, leaf0, point=None, pub=None, tensor=False):
        """The verifier's public-polynomial loop on the host, by value (no GPU): (n_queries, 2, 64, 2) uint64 — [q, 0, j] = q_j(w^leaf0[q]),
        [q, 1, j] = q_j(-w^leaf0[q]).  point: (n, 2) uint64, the public vector is eq(point, .); pub: (2^n, 2), a general vector; tensor: the point
        form through one transform.  Raises ValueError on refused arguments."""
        import numpy as np
        lf = np.ascontiguousarray(leaf0, dtype=np.uint64).reshape(-1)
        pt = None if point is None else np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 2)
        pb = None if pub is None else np.ascontiguousarray(pub, dtype=np.uint64).reshape(-1, 2)
        if (pt is not None and pt.shape[0] != n) or (pb is not None and (n < 0 or n > 30 or pb.shape[0] != 1 << n)):
            raise ValueError("pc_public_evals_host: a point of n coordinates or a vector of 2^n entries")
        out = np.zeros((max(len(lf), 1), 2, 64, 2), dtype=np.uint64)
        rc = lib_host().vph_pc_public_evals_host(int(n), None if pt is None else pt.ctypes.data, None if pb is None else pb.ctypes.data, 1 if tensor else 0,
                                                 len(lf), lf.ctypes.data, out.ctypes.data)
        if rc:
            raise ValueError("pc_public_evals_host: refused")
        return out[: len(lf)]

    @staticmethod
    def pc_opening_digests_host(n, leaf0, answer):
        """The verifier's opening-digest loop on the host, by value (no GPU): answer = bytes in vp_fri_query's layout for (n, len(leaf0)); returns
        64 bytes per opening, in the layout's order: recomputed leaf-chain digest | root reached through the path.  Raises ValueError when refused."""
        import numpy as np
        lf = np.ascontiguousarray(leaf0, dtype=np.uint64).reshape(-1)
        buf = ctypes.create_string_buffer(bytes(answer), max(len(answer), 1))
        out = ctypes.create_string_buffer(max(len(lf) * max(n - 4, 0) * 64, 1))
        if lib_host().vph_pc_opening_digests_host(int(n), len(lf), lf.ctypes.data, ctypes.cast(buf, ctypes.c_void_p), len(answer), ctypes.cast(out, ctypes.c_void_p)):
            raise ValueError("pc_opening_digests_host: refused")
        return out.raw[: len(lf) * (n - 4) * 64]

    @staticmethod
    def pc_mask_evals_host(n, leaf0, pub_mask, ms):
        """The mask row of the verifier's public evaluation on the host, by value (no GPU): (n_queries, 2, 2) uint64 — [q, h] = the public mask polynomial (the
        interpolant of pub_mask, zero-padded to ms, on the ms-th roots of unity) at (-1)^h w^leaf0[q].  Raises ValueError on refused arguments."""
        import numpy as np
        lf = np.ascontiguousarray(leaf0, dtype=np.uint64).reshape(-1)
        pm = np.ascontiguousarray(pub_mask, dtype=np.uint64).reshape(-1, 2)
        out = np.zeros((max(len(lf), 1), 2, 2), dtype=np.uint64)
        if lib_host().vph_pc_mask_evals_host(int(n), pm.ctypes.data if pm.shape[0] else None, pm.shape[0], int(ms), len(lf), lf.ctypes.data, out.ctypes.data):
            raise ValueError("pc_mask_evals_host: refused")
        return out[: len(lf)]

    @staticmethod
    def verify_commitment(n, claim, root_l, root_h, all_sum, r, fri_roots, final_code, final_mask, leaf0, answer, point=None, pub=None, pub_mask=None, ms=1,
                          device=None):
        """The commitment's verifier by value (vph_verify_commitment, host/vphost.h): no session, no circuit.  Field elements as (k, 2) uint64 arrays (claim:
        (2,)), roots and the answer block (vp_fri_query's layout for (n, len(leaf0))) as bytes; exactly one of point / pub; pub_mask with ms, the private mask's
        padded length (1: the zero mask).  device=k: the heavy loops on GPU k, same verdict.  Returns (accepted, reason) — reason names the failed check;
        raises ValueError on malformed arguments and RuntimeError when the device could not run the loops."""
        import numpy as np
        arr = lambda a, rows: np.ascontiguousarray(a, dtype=np.uint64).reshape(rows, 2)
        lf = np.ascontiguousarray(leaf0, dtype=np.uint64).reshape(-1)
        pt = None if point is None else arr(point, -1)
        pb = None if pub is None else arr(pub, -1)
        pm = None if pub_mask is None else arr(pub_mask, -1)
        if (pt is not None and pt.shape[0] != n) or (pb is not None and (n < 0 or n > 30 or pb.shape[0] != 1 << n)):
            raise ValueError("verify_commitment: a point of n coordinates or a vector of 2^n entries")
        if n < 7 or len(root_l) != 32 or len(root_h) != 32 or len(fri_roots) != 32 * (n - 6):
            raise ValueError("verify_commitment: n >= 7, roots of 32 bytes, n - 6 FRI roots")
        cl, sums, rr, fc, fm = arr(claim, 1), arr(all_sum, 65), arr(r, n - 6), arr(final_code, 2048), arr(final_mask, 32)
        keep = [ctypes.create_string_buffer(bytes(b), max(len(b), 1)) for b in (root_l, root_h, fri_roots, answer)]
        cp = lambda b: ctypes.cast(b, ctypes.c_void_p)
        err = ctypes.create_string_buffer(512)
        rc = lib_host().vph_verify_commitment(int(n), None if pt is None else pt.ctypes.data, None if pb is None else pb.ctypes.data,
                                              None if pm is None or not pm.shape[0] else pm.ctypes.data, 0 if pm is None else pm.shape[0], int(ms), cl.ctypes.data,
                                              cp(keep[0]), cp(keep[1]), sums.ctypes.data, rr.ctypes.data, cp(keep[2]), fc.ctypes.data, fm.ctypes.data, len(lf),
                                              lf.ctypes.data, cp(keep[3]), len(answer), -1 if device is None else int(device), err, len(err))
        if rc == -1:
            raise ValueError("verify_commitment: " + err.value.decode())
        if rc < 0:
            raise RuntimeError("verify_commitment: " + err.value.decode())
        return rc == 0, err.value.decode() if rc else ""

    @staticmethod
    def verify_commitment_fs(proof, device=None, min_pow_bits=0):
        """Verify a non-interactive commitment proof (Session.commit_fs; layout and chain: host/vphost.h): no tape, no session, no circuit.  The fold challenges
        and query positions are derived from the proof itself, then verify_commitment's checks run unchanged.  device=k: the heavy loops on GPU k.  Returns
        (accepted, reason); raises ValueError on a malformed proof and RuntimeError when the device could not run the loops.  min_pow_bits: the proof of work
        the verifier demands (commit_fs(pow_bits=)); a proof that carries less, or whose work is not met, is rejected."""
        proof = bytes(proof)
        buf = ctypes.create_string_buffer(proof, max(len(proof), 1))
        err = ctypes.create_string_buffer(512)
        rc = lib_host().vph_verify_commitment_fs_min(ctypes.cast(buf, ctypes.c_void_p), len(proof), -1 if device is None else int(device), int(min_pow_bits), err, len(err))
        if rc == -1:
            raise ValueError("verify_commitment_fs: " + err.value.decode())
        if rc < 0:
            raise RuntimeError("verify_commitment_fs: " + err.value.decode())
        return rc == 0, err.value.decode() if rc else ""

    @staticmethod
    def commitment_fs_challenges(proof):
        """The derivation alone: (r, leaf0) of a well-formed commitment proof — the n - 6 fold challenges as an (n - 6, 2) uint64 array and the positions as a
        list.  Raises ValueError on a malformed proof."""
        import struct
        import numpy as np
        proof = bytes(proof)
        if len(proof) < 32:
            raise ValueError("commitment_fs_challenges: malformed proof")
        n, reps = struct.unpack_from("<II", proof, 8)
        if not (7 <= n <= 30 and 1 <= reps <= 4096):
            raise ValueError("commitment_fs_challenges: malformed proof")
        buf = ctypes.create_string_buffer(proof, len(proof))
        r, lf = np.zeros((n - 6, 2), np.uint64), np.zeros(reps, np.uint64)
        if lib_host().vph_commitment_fs_challenges(ctypes.cast(buf, ctypes.c_void_p), len(proof), r.ctypes.data, lf.ctypes.data):
            raise ValueError("commitment_fs_challenges: malformed proof")
        return r, [int(x) for x in lf]

    @staticmethod
    def fs_pow(proof):
        """(pow_bits, nonce) of a commitment proof or a joined proof, read from its header (vph_fs_pow): (0, 0) for a version-1 proof.  Raises ValueError on a
        malformed header."""
        proof = bytes(proof)
        buf = ctypes.create_string_buffer(proof, max(len(proof), 1))
        bits, nonce = ctypes.c_uint64(0), ctypes.c_uint64(0)
        if lib_host().vph_fs_pow(ctypes.cast(buf, ctypes.c_void_p), len(proof), ctypes.byref(bits), ctypes.byref(nonce)):
            raise ValueError("fs_pow: malformed proof")
        return int(bits.value), int(nonce.value)

    def verify_full_fs(self, proof, device=None, return_point=False, min_pow_bits=0):
        """Verify a joined non-interactive proof of the whole protocol (Session.prove_full_fs; chain and layout: host/vphost.h, "The joined proof") holding only this
        circuit: no tape, no session, no input values.  device=k: the commitment's heavy loops on GPU k.  Returns (accepted, reason) — with return_point also the
        derived point as an (n, 2) uint64 array (a rejected GKR part: as far as its replay got); raises ValueError on a malformed proof and RuntimeError without the device.
        min_pow_bits: the proof of work the verifier demands (prove_full_fs(pow_bits=)); a proof that carries less, or whose work is not met, is rejected."""
        import numpy as np
        proof = bytes(proof)
        buf = ctypes.create_string_buffer(proof, max(len(proof), 1))
        err = ctypes.create_string_buffer(512)
        n = self.layer_bitlen(0)
        pt = np.full((max(n, 1), 2), (1 << 64) - 1, np.uint64)
        rc = lib_host().vph_verify_full_fs_min(self.h, ctypes.cast(buf, ctypes.c_void_p), len(proof), -1 if device is None else int(device), int(min_pow_bits), pt.ctypes.data,
                                               err, len(err))
        if rc == -1:
            raise ValueError("verify_full_fs: " + err.value.decode())
        if rc < 0:
            raise RuntimeError("verify_full_fs: " + err.value.decode())
        out = (rc == 0, err.value.decode() if rc else "")
        return out + (None if int(pt[0, 0]) == (1 << 64) - 1 else pt,) if return_point else out

    @staticmethod
    def fft_gkr_fs_tape(lg, state, msgs):
        """fft_gkr's part of the Fiat-Shamir chain, the derivation alone (vph_fft_gkr_fs_tape, host/vphost.h): from the 32-byte chain state and the messages
        of fft_gkr(lg) in vp_fft_gkr's layout, the tape the device drew as an (n_tape, 2) uint64 array and the closing state.  No GPU.  Raises ValueError on
        lg outside 1..19, a wrong message count or a non-canonical limb."""
        import numpy as np
        state = bytes(state)
        m = np.ascontiguousarray(msgs, dtype=np.uint64).reshape(-1, 2)
        lg = int(lg)
        if len(state) != 32 or not 1 <= lg <= 19:
            raise ValueError("fft_gkr_fs_tape: bad arguments")
        tape = np.zeros((2 * lg * lg + 9 * lg + 96, 2), np.uint64)
        st_in, st_out = ctypes.create_string_buffer(state, 32), ctypes.create_string_buffer(32)
        if lib_host().vph_fft_gkr_fs_tape(lg, ctypes.cast(st_in, ctypes.c_void_p), m.ctypes.data, m.shape[0], tape.ctypes.data, ctypes.cast(st_out, ctypes.c_void_p)):
            raise ValueError("fft_gkr_fs_tape: malformed messages")
        return tape, st_out.raw

    @staticmethod
    def fft_gkr_check(lg, tape, msgs):
        """The host verifier of fft_gkr (fft_gkr_check, host/fft_gkr_verify.hpp) on a tape and messages by value: True iff every check holds.  Raises
        ValueError on malformed arrays."""
        import numpy as np
        t = np.ascontiguousarray(tape, dtype=np.uint64).reshape(-1, 2)
        m = np.ascontiguousarray(msgs, dtype=np.uint64).reshape(-1, 2)
        rc = lib_host().vph_fft_gkr_check(int(lg), t.ctypes.data, t.shape[0], m.ctypes.data, m.shape[0])
        if rc < 0:
            raise ValueError("fft_gkr_check: malformed tape or messages")
        return rc == 0

    def gkr_sizes(self):
        """(tape elements, transcript bytes) of the circuit's GKR part (vph_gkr_sizes): the sizes of vp_prove_gkr and vp_prove_gkr_fs.  No GPU."""
        nt, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        if lib_host().vph_gkr_sizes(self.h, ctypes.byref(nt), ctypes.byref(nb)):
            raise ValueError("gkr_sizes: a circuit of at least two layers")
        return int(nt.value), int(nb.value)

    def gkr_fs_tape(self, transcript, state):
        """The GKR part of the Fiat-Shamir chain, the derivation alone (vph_gkr_fs_tape; the schedule: host/vphost.h, "The GKR part on the device"): from the
        32-byte chain state and a GKR transcript in vp_prove_gkr's layout, the tape Session.prove_gkr_fs draws as an (n_tape, 2) uint64 array (slots the
        schedule never draws zero), the number of draws and the closing state.  A walk over the bytes: nothing is verified.  No GPU.  Raises ValueError on a
        state that is not 32 bytes, a transcript of another length than the circuit's, or a non-canonical limb."""
        import numpy as np
        state, transcript = bytes(state), bytes(transcript)
        nt, nb = self.gkr_sizes()
        if len(state) != 32 or len(transcript) != nb:
            raise ValueError("gkr_fs_tape: a 32-byte state and a transcript of %d bytes" % nb)
        tape = np.zeros((nt, 2), np.uint64)
        st_in, st_out = ctypes.create_string_buffer(state, 32), ctypes.create_string_buffer(32)
        buf = ctypes.create_string_buffer(transcript, max(len(transcript), 1))
        nd = ctypes.c_uint64(0)
        if lib_host().vph_gkr_fs_tape(self.h, ctypes.cast(st_in, ctypes.c_void_p), ctypes.cast(buf, ctypes.c_void_p), len(transcript), tape.ctypes.data, ctypes.byref(nd),
                                      ctypes.cast(st_out, ctypes.c_void_p)):
            raise ValueError("gkr_fs_tape: malformed transcript")
        return tape, int(nd.value), st_out.raw

    def verify_fs(self, proof):
        """Verify a Fiat-Shamir proof (Session.prove_fs) on the host: no GPU, no tape."""
        buf = ctypes.create_string_buffer(bytes(proof), len(proof))
        return lib_host().vph_verify_fs(self.h, ctypes.cast(buf, ctypes.c_void_p), len(proof)) == 0

    def close(self):
        if self.h:
            lib_host().vph_circuit_free(self.h)
            self.h = None


_PUBLIC_OPTIONS = ("use_graph", "plan_autotune", "real_values", "real_pairs", "pc_tensor_pub", "persistent_rounds", "persistent_timeout_ms", "poll", "prefetch_round1",
                   "interactive_fast_init", "split_cost_percent", "debug")
# internal tuning knobs (csrc/vpgpu.hip, VpOpt): name -> the VP_* environment variable the library reads once per vp_create (tests / benches / A-B only)
_TUNING_ENV = {"gkr_path": "VP_GKR_PATH", "serial": "VP_GKR_SERIAL", "fuse_init": "VP_FUSE_INIT", "fuse_min_log": "VP_FUSE_MIN_LOG", "fuse_dot": "VP_FUSE_DOT",
               "drop_y": "VP_DROP_Y", "drop_y_round1": "VP_DROP_Y1", "seg_tiny": "VP_SEG_TINY", "sf_big_log": "VP_SF_BIG_LOG", "sf3b_grid": "VP_SF3B_GRID",
               "dot_blocks": "VP_DOT_BLOCKS", "plan_align": "VP_PLAN_ALIGN", "round_fused_max": "VP_ROUND_FUSED_MAX",
               "kernel_copies": "VP_KERNEL_COPIES", "fold_branches": "VP_FOLD_BRANCHES", "fuse_combine": "VP_FUSE_COMBINE",
               "graph_explicit": "VP_GRAPH_EXPLICIT", "ntt_r8": "VP_NTT_R8", "fuse_p2": "VP_FUSE_P2", "leaf_asm": "VP_LEAF_ASM",
               "fft_gkr_batched": "VP_FFT_GKR_BATCHED", "split_vu": "VP_SPLIT_VU", "pc_live": "VP_PC_LIVE",
               "grind_window_log": "VP_GRIND_WINDOW_LOG", "grind_batch": "VP_GRIND_BATCH", "gen_rec": "VP_GEN_REC"}
VP_OPTIONS_ABI = 0x76700005


class Options(ctypes.Structure):
    """vp_options of include/vpgpu.h — what a caller can sensibly choose about how the library computes (never what).  Options() holds the shipped defaults.
    Keywords that are not fields of the struct but INTERNAL tuning knobs (the names of csrc/vpgpu.hip's VpOpt: fuse_combine, sf3b_grid, ntt_r8, gkr_path ...)
    are accepted too, for the tests: Session() sets the VP_* environment variable of each around its vp_create, which is the only way the library takes them."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("abi", ctypes.c_uint32)] + [(n, ctypes.c_int32) for n in _PUBLIC_OPTIONS] + [("reserved", ctypes.c_int32 * 4)]

    def __init__(self, **kw):
        super().__init__()
        lib_gpu().vp_options_default(ctypes.byref(self))
        self.tuning = {}
        for k, v in kw.items():
            if k in _PUBLIC_OPTIONS:
                setattr(self, k, v)
            elif k in _TUNING_ENV:
                self.tuning[k] = v
            else:
                raise TypeError("unknown option " + k)

    def tuning_env(self):
        env = {}
        for k, v in getattr(self, "tuning", {}).items():
            if k == "gkr_path":
                v = {PATH_PLAN: "plan", PATH_LANES: "lanes", PATH_SIMPLE: "simple"}[v]
            elif k == "plan_align":
                v = {0: "", 1: "left", 2: "right"}[v]
            env[_TUNING_ENV[k]] = str(v)
        return env


PATH_PLAN, PATH_LANES, PATH_SIMPLE = 0, 1, 3


class Session:
    """One prover on one GPU: circuit resident in HBM, witness evaluated on the device.

    devices + round_shard_min_log: the interactive sumchecks of one proof sharded by index over len(devices) ranks (1, 2, 4 or 8; a device may
    repeat), one context per rank (include/vpgpu.h: vp_set_round_shard).  The prove_* calls work unchanged; `device` is then ignored.

    shard_commitment=True (with devices): the Virgo commitment is sharded over the same ranks as well (vp_pc_set_shard) — commit_private / commit_public /
    commit_public_eq, the FRI commit phase and every opening run on all ranks, so prove_full, prove_and_verify_full, fri_commit, fri_open_many and
    fri_query work unchanged.  Raises when the input layer is too short for the ranks; masks and prove_protocol are not available on such a session."""

    def __init__(self, circuit, device=0, options=None, devices=None, round_shard_min_log=None, shard_commitment=False):
        err = ctypes.create_string_buffer(512)
        if (devices is None) != (round_shard_min_log is None):
            raise ValueError("Session: devices and round_shard_min_log go together")
        if shard_commitment and devices is None:
            raise ValueError("Session: shard_commitment needs devices and round_shard_min_log")
        self._shard_pc = bool(shard_commitment) and len(devices) > 1
        self.circuit = circuit
        keep = {}
        for k, v in (options.tuning_env() if options is not None else {}).items():          # internal knobs: the library reads them from the environment at vp_create
            keep[k] = os.environ.get(k)
            os.environ[k] = v
        try:
            opt = ctypes.byref(options) if options is not None else None
            if devices is None:
                self.h = lib_host().vph_session_create_opts(circuit.h, device, opt, err, len(err))
            else:
                devs = (ctypes.c_int * max(1, len(devices)))(*devices)
                self.h = lib_host().vph_session_create_sharded(circuit.h, devs, len(devices), int(round_shard_min_log), 1 if shard_commitment else 0, opt,
                                                               err, len(err))
        finally:
            for k, v in keep.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        if not self.h:
            raise RuntimeError("Session: " + err.value.decode())
        self._cap = int(lib_host().vph_transcript_bytes(self.h)) + 4096
        self._buf = ctypes.create_string_buffer(self._cap)

    def gpu_ctx(self):
        """The vp_ctx* of this session (for direct C-ABI calls in tests)."""
        return ctypes.c_void_p(lib_host().vph_session_ctx(self.h))

    def set_profiling(self, level):
        lib_host().vph_set_profiling(self.h, level)

    def launch_stats(self):
        """Per-launch table of the last profiled call (set_profiling(1), then prove_gkr / commit_private / commit_public /
        fri_commit): list of dicts {kernel, step, workgroups, jobs, rounds, first_round, bytes, work, us}."""
        ctx = lib_host().vph_session_ctx(self.h)
        n = ctypes.c_int(0)
        lib_gpu().vp_get_launch_stats(ctx, None, 0, ctypes.byref(n))
        arr = (LaunchStat * max(1, n.value))()
        lib_gpu().vp_get_launch_stats(ctx, arr, n.value, ctypes.byref(n))
        out = []
        for i in range(n.value):
            e = arr[i]
            out.append({"kernel": lib_gpu().vp_kernel_name(e.kind).decode(), "step": e.step, "workgroups": e.workgroups, "jobs": e.jobs,
                        "rounds": e.rounds, "first_round": e.first_round, "bytes": e.bytes, "work": e.work, "us": e.us})
        return out

    def gen_jobs(self):
        """Fused-init jobs of the launch plan the last prove_gkr ran, by what they generate: {mode: (row-pointer form, row-record form)} for mode
        1 (phase-1 init), 2 (Liu gather), 3 (phase-2 init); vp_get_gen_jobs."""
        out = (ctypes.c_uint32 * 8)()
        err = lib_gpu().vp_get_gen_jobs(lib_host().vph_session_ctx(self.h), out)
        if err:
            raise RuntimeError("vp_get_gen_jobs failed: %d" % err)
        return {m: (int(out[m]), int(out[4 + m])) for m in (1, 2, 3)}

    def world(self):
        """Ranks of a round-sharded session (1 otherwise)."""
        return int(lib_host().vph_session_world(self.h))

    def rank_ctx(self, rank):
        """The vp_ctx* of one rank of a round-sharded session (rank 0 = gpu_ctx())."""
        return ctypes.c_void_p(lib_host().vph_session_rank_ctx(self.h, rank))

    def partials(self):
        """Round-sharded session: every rank's partial polynomial of every round since the last clear_partials(), as a uint64 array of shape
        (rounds, world, 3, 2) — canonical limbs {real, img}."""
        import numpy as np
        n = lib_host().vph_session_partials(self.h, None, 0)
        out = np.zeros((max(1, n), 3, 2), dtype=np.uint64)
        n = lib_host().vph_session_partials(self.h, out.ctypes.data, n)
        w = self.world()
        return out[:n].reshape(n // w, w, 3, 2)

    def clear_partials(self):
        lib_host().vph_session_clear_partials(self.h)

    def drop_rank(self, rank):
        """Round-sharded session: leave this rank's partial polynomial out of the sum (-1: none) — a test of the verifier's check."""
        lib_host().vph_session_drop_rank(self.h, rank)

    def gather_sec(self):
        """Round-sharded session: host seconds spent in the gathers so far."""
        return float(lib_host().vph_session_gather_sec(self.h))

    def round_stats(self, rank=0):
        """Interactive path, one dict per vp_round since the last prove_interactive() started: {phase, layer, round, how, tables, bytes, us}
        (include/vpgpu.h: vp_round_stat — algorithmic bytes of the round by SURVEY §8d and the wall time of the call).  rank: of a round-sharded session."""
        ctx = lib_host().vph_session_rank_ctx(self.h, rank)
        n = ctypes.c_int(0)
        lib_gpu().vp_get_round_stats(ctx, None, 0, ctypes.byref(n))
        arr = (RoundStat * max(1, n.value))()
        lib_gpu().vp_get_round_stats(ctx, arr, n.value, ctypes.byref(n))
        return [{"phase": e.phase, "layer": e.layer, "round": e.round, "how": e.how, "tables": e.tables, "bytes": e.bytes, "us": e.us}
                for e in (arr[i] for i in range(n.value))]

    def comm_count(self):
        """ncclCommCount of the communicator attached with attach_comm()."""
        n = ctypes.c_int(0)
        if lib_gpu().vp_comm_count(lib_host().vph_session_ctx(self.h), ctypes.byref(n)):
            raise RuntimeError("vp_comm_count failed")
        return n.value

    def layer_values(self, layer):
        import numpy as np
        n = self.circuit.layer_size(layer)
        out = np.zeros((n, 2), dtype=np.uint64)
        rc = lib_host().vph_layer_values(self.h, layer, out.ctypes.data, n)
        if rc:
            raise RuntimeError("layer_values failed")
        return out

    def _call(self, fn):
        # per-session scratch objects: the batched proof is sub-millisecond, so ctypes allocations per call would show up
        if not hasattr(self, "_n"):
            self._n = ctypes.c_uint64(0)
            self._res = VphResult()
            self._err = ctypes.create_string_buffer(512)
            self._bufp = ctypes.cast(self._buf, ctypes.c_void_p)
        n, res, err = self._n, self._res, self._err
        rc = fn(self.h, self._bufp, self._cap, ctypes.byref(n), ctypes.byref(res), err, 512)
        if rc < 0:
            raise RuntimeError("prover failed: " + err.value.decode())
        return ctypes.string_at(self._buf, n.value), res.as_dict(), rc

    def prove_interactive(self):
        """F::init() + verifier::verify(): returns (transcript bytes, stats, verified)."""
        tr, res, rc = self._call(lib_host().vph_prove_interactive)
        b = (ctypes.c_double * 3)()
        lib_host().vph_interactive_breakdown(self.h, b)
        res["init_sec"], res["round_sec"], res["finalize_sec"] = b[0], b[1], b[2]
        return tr, res, rc == 0

    def prove_fs(self, device_draws=False):
        """Non-interactive GKR proof (Fiat-Shamir over SHA3-256): returns (proof bytes, stats, accepted by the built-in verifier).
        device_draws: the prover alone in one device pass (vph_prove_fs_ex with VPH_FS_DEVICE_GKR, vp_prove_gkr_fs) — every challenge drawn on the device, the
        same bytes; nothing is verified and the third value is None: Circuit.verify_fs is the check.  Not on a sharded session."""
        if device_draws:
            tr, res, _ = self._call(lambda h, buf, cap, n, r, err, errlen: lib_host().vph_prove_fs_ex(h, buf, cap, n, r, 2, err, errlen))
            return tr, res, None
        tr, res, rc = self._call(lib_host().vph_prove_fs)
        return tr, res, rc == 0

    def prove_gkr_fs(self, state):
        """The GKR part non-interactive on the session's GPU (vp_prove_gkr_fs, include/vpgpu.h): every challenge is drawn on the device from the Fiat-Shamir
        chain that starts at the 32-byte `state`.  Returns (transcript bytes, tape, n_draws, state_out): the transcript in prove_gkr's layout, the draws in
        prove_gkr's tape slots as an (n_tape, 2) uint64 array, their number, the closing state as bytes.  The host re-derives tape, count and state from the
        transcript (Circuit.gkr_fs_tape's walk) and raises if the device's differ.  Not on a sharded session."""
        import numpy as np
        state = bytes(state)
        if len(state) != 32:
            raise ValueError("prove_gkr_fs: a 32-byte state")
        nt, nb = self.circuit.gkr_sizes()
        tape = np.zeros((nt, 2), np.uint64)
        buf = ctypes.create_string_buffer(max(nb, 1))
        st_in, st_out = ctypes.create_string_buffer(state, 32), ctypes.create_string_buffer(32)
        n, nd = ctypes.c_uint64(0), ctypes.c_uint64(0)
        err = ctypes.create_string_buffer(512)
        rc = lib_host().vph_prove_gkr_fs(self.h, ctypes.cast(st_in, ctypes.c_void_p), ctypes.cast(buf, ctypes.c_void_p), nb, ctypes.byref(n), tape.ctypes.data, ctypes.byref(nd),
                                         ctypes.cast(st_out, ctypes.c_void_p), err, len(err))
        if rc:
            raise RuntimeError("prove_gkr_fs failed: " + err.value.decode())
        return buf.raw[: n.value], tape, int(nd.value), st_out.raw

    def draw_tape(self):
        lib_host().vph_draw_tape(self.h)

    def set_tape(self, tape):
        """Attach the caller's tape, an (n, 2) uint64 array in draw order (include/vpgpu.h: vp_prove_gkr), in place of draw_tape()'s.  Raises, and keeps the
        attached tape, when the length is not the circuit's draw count or a limb is >= p."""
        import numpy as np
        t = np.ascontiguousarray(tape, dtype=np.uint64).reshape(-1, 2)
        if lib_host().vph_set_tape(self.h, t.ctypes.data, int(t.shape[0])):
            raise ValueError("set_tape: wrong length or a non-canonical limb")

    def prove_gkr(self):
        """One batched device pass from the attached tape: returns (transcript bytes, stats)."""
        tr, res, _ = self._call(lib_host().vph_prove_gkr)
        return tr, res

    def commit_device_ms(self):
        """Device milliseconds (HIP events) of the last commit_private / commit_public / fri_commit call."""
        return float(lib_host().vph_commit_device_ms(self.h))

    def tail_resumes(self):
        """vp_get_resident_resumes: relaunches of this session's resident round kernel on a saved phase."""
        n = ctypes.c_uint64(0)
        if lib_gpu().vp_get_resident_resumes(lib_host().vph_session_ctx(self.h), ctypes.byref(n)):
            raise RuntimeError("vp_get_resident_resumes failed")
        return int(n.value)

    def options_in_effect(self):
        """vp_get_options: the configuration this session runs with (after the plan tuner, once a proof has run)."""
        import types
        o = Options()
        ctx = lib_host().vph_session_ctx(self.h)
        if lib_gpu().vp_get_options(ctx, ctypes.byref(o)):
            raise RuntimeError("vp_get_options failed")
        eff = types.SimpleNamespace(**{k: getattr(o, k) for k in _PUBLIC_OPTIONS})
        v = ctypes.c_int32(0)
        for name in _TUNING_ENV:                               # the internal knobs, by name (vp_tuning_get)
            if lib_gpu().vp_tuning_get(ctx, name.encode(), ctypes.byref(v)) == 0:
                setattr(eff, name, v.value)
        return eff

    def set_shard(self, rank, world):
        """One proof over `world` GPUs: prove_gkr() then runs only the sumcheck chains dealt to `rank` and leaves the rest of the
        transcript zero; sum_transcripts() of all ranks' outputs (one all-reduce) is the proof.  world=1 undoes it."""
        if lib_host().vph_set_shard(self.h, rank, world):
            raise RuntimeError("set_shard(%d, %d) refused" % (rank, world))

    def attach_comm(self, rank, world):
        """RCCL communicator inside the library (include/vpgpu.h: vp_comm_unique_id / vp_comm_init): rank 0 makes the id, the default
        torch.distributed group only carries those 128 bytes (control plane).  From then on a sharded prove_gkr() all-reduces the
        transcript (and the export area of an index-split proof) on the device, inside the call, and returns the finished transcript on
        every rank — no torch tensor and no host bounce on the data path."""
        import numpy as np
        import torch
        import torch.distributed as dist
        L = lib_gpu()
        uid = ctypes.create_string_buffer(128)
        if rank == 0 and L.vp_comm_unique_id(ctypes.cast(uid, ctypes.c_void_p)):
            raise RuntimeError("vp_comm_unique_id failed (librccl.so.1 not found?)")
        t = torch.from_numpy(np.frombuffer(uid.raw, dtype=np.uint8).copy())
        if "nccl" in dist.get_backend():
            t = t.cuda()
        dist.broadcast(t, src=0)
        idb = ctypes.create_string_buffer(t.cpu().numpy().tobytes(), 128)
        ctx = lib_host().vph_session_ctx(self.h)
        if L.vp_comm_init(ctx, ctypes.cast(idb, ctypes.c_void_p), rank, world):
            raise RuntimeError("vp_comm_init failed: " + (L.vp_last_error(ctx) or b"").decode())

    def set_shard_split(self, min_log):
        """On top of set_shard: tables of at least 2^(log2 W + min_log) entries are also split by index over the ranks (include/vpgpu.h:
        vp_set_shard_split); prove_gkr() then returns the rank's partial transcript followed by its export area, and
        shard_finish(sum_transcripts(parts)) is the proof.  min_log=0 switches it off."""
        ctx = lib_host().vph_session_ctx(self.h)
        L = lib_gpu()
        if L.vp_set_shard_split(ctx, int(min_log)):
            raise RuntimeError("set_shard_split(%d) refused" % min_log)
        n = ctypes.c_uint64(0)
        L.vp_gkr_sizes(ctx, None, ctypes.byref(n))
        if int(n.value) + 4096 > self._cap:
            self._cap = int(n.value) + 4096
            self._buf = ctypes.create_string_buffer(self._cap)
            if hasattr(self, "_n"):
                self._bufp = ctypes.cast(self._buf, ctypes.c_void_p)

    def shard_vu_partials(self):
        """Index-split proof without a communicator: this rank's partial inner products for the V_u of the split phase-2 chains (include/vpgpu.h:
        vp_shard_vu_partials) as a numpy array of shape (n, 2), uint64; n may be 0."""
        import numpy as np
        cap = max(1, int(self.circuit.layers))
        out = np.zeros((cap, 2), dtype=np.uint64)
        n = lib_host().vph_shard_vu_partials(self.h, out.ctypes.data, cap)
        if n < 0:
            raise RuntimeError("shard_vu_partials refused")
        return out[:n].copy()

    def shard_vu_set(self, sums):
        """... and their u64 sum over the ranks, for this rank's next prove_gkr() (vp_shard_vu_set)."""
        import numpy as np
        a = np.ascontiguousarray(sums, dtype=np.uint64).reshape(-1, 2)
        if lib_host().vph_shard_vu_set(self.h, a.ctypes.data, int(a.shape[0])):
            raise RuntimeError("shard_vu_set refused")

    def shard_finish(self, summed):
        """The transcript of an index-split proof from the u64 sum of the ranks' prove_gkr() outputs (vp_shard_finish)."""
        ctx = lib_host().vph_session_ctx(self.h)
        buf = ctypes.create_string_buffer(bytes(summed), len(summed))
        n = ctypes.c_uint64(0)
        if lib_gpu().vp_shard_finish(ctx, buf, len(summed), ctypes.byref(n)):
            raise RuntimeError("shard_finish refused")
        return buf.raw[:int(n.value)]

    def shard_chains(self):
        """(owner rank, cost estimate) per sumcheck chain of the proof, in plan order (include/vpgpu.h: vp_shard_chains)."""
        import numpy as np
        cap = 3 * self.circuit.layers + 1
        owner = np.zeros(cap, dtype=np.int32)
        cost = np.zeros(cap, dtype=np.float64)
        n = lib_host().vph_shard_chains(self.h, owner.ctypes.data, cost.ctypes.data, cap)
        if n < 0:
            raise RuntimeError("shard_chains failed")
        return owner[:n].copy(), cost[:n].copy()

    def commit_private(self, mask=None):
        """prover::commit_private(): (32-byte Merkle root, device milliseconds).  mask: (k, 2) uint64, the mask vector of lib/virgo's
        commit_private_array (a non-zero one fills the 65th slice; refused on a sharded commitment)."""
        root = ctypes.create_string_buffer(32)
        ms = ctypes.c_double(0)
        err = ctypes.create_string_buffer(512)
        if mask is not None:
            import numpy as np
            mask = np.ascontiguousarray(mask, dtype=np.uint64).reshape(-1, 2)
            rc = lib_host().vph_commit_private_masked(self.h, mask.ctypes.data, mask.shape[0], ctypes.cast(root, ctypes.c_void_p), ctypes.byref(ms), err, len(err))
        else:
            rc = lib_host().vph_commit_private(self.h, ctypes.cast(root, ctypes.c_void_p), ctypes.byref(ms), err, len(err))
        if rc:
            raise RuntimeError("commit_private failed: " + err.value.decode())
        return root.raw, ms.value

    def commit_public(self, pub):
        """prover::commit_public on a (2^n, 2) uint64 array: (root_h, input_0 bytes, all_sum bytes, device ms)."""
        import numpy as np
        pub = np.ascontiguousarray(pub, dtype=np.uint64)
        out = ctypes.create_string_buffer(32 + 16 + 65 * 16)
        ms = ctypes.c_double(0)
        err = ctypes.create_string_buffer(512)
        rc = lib_host().vph_commit_public(self.h, pub.ctypes.data, pub.shape[0], ctypes.cast(out, ctypes.c_void_p), ctypes.byref(ms),
                                          err, len(err))
        if rc:
            raise RuntimeError("commit_public failed: " + err.value.decode())
        return out.raw[:32], out.raw[32:48], out.raw[48:], ms.value

    def prove_full(self, batched=False):
        """commit_private + GKR + commit_public: the full golden transcript layout; returns (bytes, verified)."""
        cap = self._cap + 32 + 32 + 16 + 65 * 16
        buf = ctypes.create_string_buffer(cap)
        n = ctypes.c_uint64(0)
        err = ctypes.create_string_buffer(512)
        rc = lib_host().vph_prove_full(self.h, ctypes.cast(buf, ctypes.c_void_p), cap, ctypes.byref(n), 1 if batched else 0, err, len(err))
        if rc < 0:
            raise RuntimeError("prove_full failed: " + err.value.decode())
        return buf.raw[: n.value], rc == 0

    def commit_public_eq(self, point, pub_mask=None):
        """prover::commit_public on pub = eq(point, .) built on the device (vp_commit_public_eq): (root_h, input_0 bytes, all_sum bytes, device ms).
        pub_mask: (k, 2) uint64, the public mask vector behind commit_private(mask) (vp_commit_public_eq_masked); behind a zero private mask it changes nothing."""
        import numpy as np
        point = np.ascontiguousarray(point, dtype=np.uint64)
        out = ctypes.create_string_buffer(32 + 16 + 65 * 16)
        if pub_mask is not None:
            pub_mask = np.ascontiguousarray(pub_mask, dtype=np.uint64).reshape(-1, 2)
            ms = ctypes.c_double(0)
            err = ctypes.create_string_buffer(512)
            if lib_host().vph_commit_public_eq_masked(self.h, point.ctypes.data, point.shape[0], pub_mask.ctypes.data, pub_mask.shape[0], ctypes.cast(out, ctypes.c_void_p),
                                                      ctypes.byref(ms), err, len(err)):
                raise RuntimeError("vp_commit_public_eq_masked failed: " + err.value.decode())
            return out.raw[:32], out.raw[32:48], out.raw[48:], ms.value
        if self._shard_pc:                                  # every rank is handed the point
            ms = ctypes.c_double(0)
            err = ctypes.create_string_buffer(512)
            if lib_host().vph_commit_public_eq(self.h, point.ctypes.data, point.shape[0], ctypes.cast(out, ctypes.c_void_p), ctypes.byref(ms), err, len(err)):
                raise RuntimeError("vp_commit_public_eq failed: " + err.value.decode())
            return out.raw[:32], out.raw[32:48], out.raw[48:], ms.value
        ctx = lib_host().vph_session_ctx(self.h)
        base = ctypes.addressof(out)
        rc = lib_gpu().vp_commit_public_eq(ctx, point.ctypes.data, point.shape[0], base + 32, base + 48, base)
        if rc:
            raise RuntimeError("vp_commit_public_eq failed: %d %s" % (rc, (lib_gpu().vp_last_error(ctx) or b"").decode()))
        return out.raw[:32], out.raw[32:48], out.raw[48:], self.commit_device_ms()

    def fs_grind(self, state, bits, first=0, max_tries=None):
        """The proof-of-work search on the session's GPU (vp_fs_grind, include/vpgpu.h): the smallest nonce in [first, first + max_tries) whose chain step
        W(bits, nonce) on the 32-byte `state` leaves the low `bits` bits of the new state's first word zero.  Returns (nonce, state_out); raises ValueError on
        arguments outside the limits and RuntimeError when the range holds no such nonce (VP_ELIMIT).  max_tries None: 64 x 2^bits."""
        state, bits, first, max_tries = _fs_grind_args(state, bits, first, max_tries)
        ctx = lib_host().vph_session_ctx(self.h)
        st_in, st_out, nonce = ctypes.create_string_buffer(state, 32), ctypes.create_string_buffer(32), ctypes.c_uint64(0)
        rc = lib_gpu().vp_fs_grind(ctx, ctypes.cast(st_in, ctypes.c_void_p), bits, first, max_tries, ctypes.byref(nonce), ctypes.cast(st_out, ctypes.c_void_p))
        if rc:
            raise RuntimeError("fs_grind failed: %d %s" % (rc, (lib_gpu().vp_last_error(ctx) or b"").decode()))
        return int(nonce.value), st_out.raw

    def commit_fs(self, point, reps=33, mask=None, pub_mask=None, device_draws=True, pow_bits=0):
        """The non-interactive commitment proof of the session's input layer at `point` (vph_commit_fs, host/vphost.h): one block of bytes for
        Circuit.verify_commitment_fs.  mask / pub_mask: the vectors of a hiding commitment, as for commit_private(mask) and commit_public_eq(pub_mask=).
        device_draws: the commit phase draws every fold challenge on the device (vp_fri_commit_fs); False: the vp_fri_step loop with the chain on the host —
        the same bytes.  pow_bits (0 .. 32): grind that many bits of proof of work in front of the query positions (a version-2 proof; the search is
        fs_grind, with device_draws=False the host's); 0: the version-1 proof.  Not on a session with a sharded commitment."""
        import numpy as np
        if not 0 <= int(pow_bits) <= 32:
            raise ValueError("commit_fs: pow_bits in 0..32")
        arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 2)
        pt, m, pm = arr(point), arr(mask), arr(pub_mask)
        ptr = lambda a: a.ctypes.data if a is not None and a.shape[0] else None
        cnt = lambda a: 0 if a is None else a.shape[0]
        n = pt.shape[0]
        cap = 4096 + 16 * (n + cnt(pm)) + 32 * n + (2048 + 32) * 16 + int(reps) * ((n - 4) * 2080 + 32 * (n * n))
        buf = ctypes.create_string_buffer(cap)
        ln = ctypes.c_uint64(0)
        err = ctypes.create_string_buffer(512)
        rc = lib_host().vph_commit_fs_pow(self.h, pt.ctypes.data, n, int(reps), ptr(m), cnt(m), ptr(pm), cnt(pm), 0 if device_draws else 1, int(pow_bits),
                                          ctypes.cast(buf, ctypes.c_void_p), cap, ctypes.byref(ln), err, len(err))
        if rc:
            raise RuntimeError("commit_fs failed: " + err.value.decode())
        return buf.raw[: ln.value]

    def prove_full_fs(self, reps=33, mask=None, pub_mask=None, return_point=False, device_gkr=False, pow_bits=0):
        """The joined non-interactive proof of the whole protocol on the session's circuit and input (vph_prove_full_fs, host/vphost.h): commit_private(mask), the GKR
        part as prove_fs with the input check left to the commitment, commit_public_eq at the derived point, fft_gkr with its challenges drawn on the device, the
        FRI commit phase, final codewords, derived positions and their openings, on one Fiat-Shamir chain — one block of bytes for Circuit.verify_full_fs.
        device_gkr: the GKR part in one device pass with its challenges drawn on the device (vp_prove_gkr_fs) instead of the verifier-driven loop: the same
        bytes; the prover's own GKR proof is then not verified on the way.  pow_bits (0 .. 32): grind that many bits of proof of work in front of the query
        positions (a version-2 proof, the search on the device); 0: the version-1 proof.  Not on a sharded session."""
        import numpy as np
        if not 0 <= int(pow_bits) <= 32:
            raise ValueError("prove_full_fs: pow_bits in 0..32")
        arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 2)
        m, pm = arr(mask), arr(pub_mask)
        ptr = lambda a: a.ctypes.data if a is not None and a.shape[0] else None
        cnt = lambda a: 0 if a is None else a.shape[0]
        err = ctypes.create_string_buffer(512)
        ln = ctypes.c_uint64(0)
        pt = np.zeros((32, 2), np.uint64)
        cap = 1 << 22
        for _ in range(2):                                     # a proof larger than the first buffer: the call reports its size and is made again
            buf = ctypes.create_string_buffer(cap)
            rc = lib_host().vph_prove_full_fs_pow(self.h, int(reps), ptr(m), cnt(m), ptr(pm), cnt(pm), ctypes.cast(buf, ctypes.c_void_p), cap, ctypes.byref(ln), pt.ctypes.data,
                                                  2 if device_gkr else 0, int(pow_bits), err, len(err))
            if rc != -1 or ln.value <= cap:
                break
            cap = ln.value
        if rc:
            raise RuntimeError("prove_full_fs failed: " + err.value.decode())
        proof = buf.raw[: ln.value]
        import struct
        return (proof, pt[:struct.unpack_from("<I", proof, 8)[0]].copy()) if return_point else proof

    def fft_gkr_fs(self, lg, state):
        """fft_gkr(lg) non-interactive on the session's GPU (vp_fft_gkr_fs, include/vpgpu.h): every challenge is drawn on the device from the Fiat-Shamir chain
        that starts at the 32-byte `state`.  Returns (msgs, tape, state_out): the messages and the tape drawn as (n, 2) uint64 arrays, the closing state as
        bytes.  The host re-derives the tape and the state from the messages and raises if the device's differ."""
        import numpy as np
        state, lg = bytes(state), int(lg)
        if len(state) != 32 or not 1 <= lg <= 19:
            raise ValueError("fft_gkr_fs: lg in 1..19 and a 32-byte state")
        msgs = np.zeros((84 + 6 * lg * lg + 8 * lg, 2), np.uint64)
        tape = np.zeros((2 * lg * lg + 9 * lg + 96, 2), np.uint64)
        st_in, st_out = ctypes.create_string_buffer(state, 32), ctypes.create_string_buffer(32)
        err = ctypes.create_string_buffer(512)
        rc = lib_host().vph_fft_gkr_fs(self.h, lg, ctypes.cast(st_in, ctypes.c_void_p), msgs.ctypes.data, msgs.shape[0], tape.ctypes.data,
                                       ctypes.cast(st_out, ctypes.c_void_p), err, len(err))
        if rc:
            raise RuntimeError("fft_gkr_fs failed: " + err.value.decode())
        return msgs, tape, st_out.raw

    def last_commit_fs_times(self):
        """(host seconds, device milliseconds) of the last commit_fs's commit phase alone"""
        out = (ctypes.c_double * 2)()
        lib_host().vph_last_commit_fs_times(self.h, out)
        return out[0], out[1]

    def warm(self):
        """vp_warm(VP_WARM_COMMITMENT | VP_WARM_FFT_GKR): the commitment's tables, buffers and pinned staging (and fft_gkr's arrays) exist before the first prover call (include/vpgpu.h)."""
        ctx = lib_host().vph_session_ctx(self.h)
        if lib_gpu().vp_warm(ctx, 3):
            raise RuntimeError("vp_warm failed: " + (lib_gpu().vp_last_error(ctx) or b"").decode())

    def draw_protocol_tape(self):
        """F::init() + every draw of verifier::verify() up front, in its order: GKR, fft_gkr, FRI fold challenges."""
        if lib_host().vph_draw_protocol_tape(self.h):
            raise RuntimeError("draw_protocol_tape: the commitment needs an input layer of at least 2^7 wires")

    def prove_protocol(self, deferred=False, queue_next=False, hash_per_call=False, mask=None, pub_mask=None):
        """The prover side of the complete protocol in one pass (no verifier work): commit_private -> batched GKR -> commit_public on
        eq(r_liu, .) -> fft_gkr -> FRI commit phase.  Returns (transcript in the golden layout, FRI roots bytes, final codeword (2048, 2),
        seconds dict {total, commit_private, gkr, commit_public, fft_gkr, fri_commit}).
        deferred: the calls are queued back to back and collected at the end (vp_set_deferred: no idle device between them); the per-call seconds are then
        device times.  queue_next: the pass also queues the next pass's commit_private behind its own folds (vphost.h, VPH_PASS_QUEUE_NEXT): for a
        session that proves back to back; this pass's commitment cannot be opened afterwards.  hash_per_call: every commit hashes its own oracle (three
        leaf-hash launches) instead of the one launch behind the FRI folds (vphost.h, VPH_PASS_HASH_PER_CALL): same bytes, the A/B partner.
        mask / pub_mask: (k, 2) uint64 mask vectors of a hiding commitment (vph_prove_protocol_masked: the 65th slice of every oracle carries them); with a
        mask given the result has a fifth element, the mask slice's final codeword (32, 2) — zeros for an all-zero mask, which is the pass without one.
        queue_next is refused together with a non-zero mask."""
        import numpy as np
        if not hasattr(self, "_pp"):
            cap = self._cap + 32 + 32 + 16 + 65 * 16
            self._pp = (ctypes.create_string_buffer(cap), cap, ctypes.create_string_buffer(32 * 32), np.zeros((2048, 2), dtype=np.uint64),
                        (ctypes.c_double * 6)(), ctypes.c_uint64(0), ctypes.create_string_buffer(512))
        buf, cap, roots, fin, sec, n, err = self._pp
        flags = (1 if deferred or queue_next else 0) | (2 if queue_next else 0) | (4 if hash_per_call else 0)
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint64).reshape(-1, 2)
            pm = np.ascontiguousarray(pub_mask if pub_mask is not None else np.zeros((0, 2)), dtype=np.uint64).reshape(-1, 2)
            fm = np.zeros((32, 2), dtype=np.uint64)
            rc = lib_host().vph_prove_protocol_masked(self.h, mask.ctypes.data, mask.shape[0], pm.ctypes.data if pm.shape[0] else None, pm.shape[0],
                                                      ctypes.cast(buf, ctypes.c_void_p), cap, ctypes.byref(n), ctypes.cast(roots, ctypes.c_void_p), len(roots),
                                                      fin.ctypes.data, fm.ctypes.data, sec, flags, err, len(err))
            if rc:
                raise RuntimeError("prove_protocol failed: " + err.value.decode())
            st = self.circuit.layer_bitlen(0) - 6
            return (buf.raw[: n.value], roots.raw[:32 * st], fin.copy(),
                    {"total": sec[0], "commit_private": sec[1], "gkr": sec[2], "commit_public": sec[3], "fft_gkr": sec[4], "fri_commit": sec[5]}, fm)
        rc = lib_host().vph_prove_protocol_ex(self.h, ctypes.cast(buf, ctypes.c_void_p), cap, ctypes.byref(n), ctypes.cast(roots, ctypes.c_void_p), len(roots),
                                              fin.ctypes.data, sec, (1 if deferred or queue_next else 0) | (2 if queue_next else 0) | (4 if hash_per_call else 0), err, len(err))
        if rc:
            raise RuntimeError("prove_protocol failed: " + err.value.decode())
        st = self.circuit.layer_bitlen(0) - 6
        return (buf.raw[: n.value], roots.raw[:32 * st], fin.copy(),
                {"total": sec[0], "commit_private": sec[1], "gkr": sec[2], "commit_public": sec[3], "fft_gkr": sec[4], "fri_commit": sec[5]})

    def prove_and_verify_full(self, reps=33, batched_openings=False, device_verifier=False, mask=None, pub_mask=None):
        """The complete protocol incl. commitment verification: (transcript bytes, accepted, times dict).  batched_openings: the query phase is
        answered in one device pass (vp_fri_query) instead of one vp_fri_open per opening; same positions, openings and checks.  device_verifier: the
        verifier's heavy loops — wiring predicates, public polynomial values, opening digests — run on the session's device (VPH_VERIFY_DEVICE_LOOPS;
        implies the one-pass query phase); every comparison stays on the host, and transcript, record and verdict are the host mode's.
        mask / pub_mask: (k, 2) uint64 mask vectors of a hiding commitment (vph_prove_and_verify_full_masked): the 65th slice is proved and verified like the
        other 64, and last_full_record() is then a version-2 record; an all-zero mask is the run without one.  A mask the device refuses raises RuntimeError."""
        cap = self._cap + 32 + 32 + 16 + 65 * 16
        buf = ctypes.create_string_buffer(cap)
        n = ctypes.c_uint64(0)
        t = [ctypes.c_double(0) for _ in range(3)]
        err = ctypes.create_string_buffer(512)
        if mask is not None:
            import numpy as np
            mk = np.ascontiguousarray(mask, dtype=np.uint64).reshape(-1, 2)
            pm = np.ascontiguousarray(pub_mask if pub_mask is not None else np.zeros((0, 2)), dtype=np.uint64).reshape(-1, 2)
            rc = lib_host().vph_prove_and_verify_full_masked(self.h, reps, (1 if batched_openings else 0) | (2 if device_verifier else 0),
                                                             mk.ctypes.data if mk.shape[0] else None, mk.shape[0], pm.ctypes.data if pm.shape[0] else None, pm.shape[0],
                                                             ctypes.cast(buf, ctypes.c_void_p), cap, ctypes.byref(n), ctypes.byref(t[0]), ctypes.byref(t[1]),
                                                             ctypes.byref(t[2]), err, len(err))
        elif batched_openings or device_verifier:
            rc = lib_host().vph_prove_and_verify_full_ex(self.h, reps, (1 if batched_openings else 0) | (2 if device_verifier else 0), ctypes.cast(buf, ctypes.c_void_p), cap, ctypes.byref(n),
                                                         ctypes.byref(t[0]), ctypes.byref(t[1]), ctypes.byref(t[2]), err, len(err))
        else:
            rc = lib_host().vph_prove_and_verify_full(self.h, reps, ctypes.cast(buf, ctypes.c_void_p), cap, ctypes.byref(n),
                                                      ctypes.byref(t[0]), ctypes.byref(t[1]), ctypes.byref(t[2]), err, len(err))
        if rc < 0:
            raise RuntimeError("prove_and_verify_full failed: " + err.value.decode())
        pt = (ctypes.c_double * 3)()
        lib_host().vph_last_pc_times(self.h, pt)
        vs = (ctypes.c_double * 4)()
        lib_host().vph_last_verify_split(self.h, vs)
        return buf.raw[: n.value], rc == 0, {"gkr_prove_sec": t[0].value, "pc_prove_sec": t[1].value, "verify_sec": t[2].value,
                                            "pc_fft_gkr_sec": pt[1], "pc_query_answer_sec": pt[2],
                                            "verify_predicates_sec": vs[0], "verify_public_eval_sec": vs[1], "verify_digests_sec": vs[2], "verify_rest_sec": vs[3]}

    def verifier_launch_stats(self):
        """With set_profiling(1): the launch tables of the verifier-side device calls of the last prove_and_verify_full (vp_predicates, vp_liu_gr,
        vp_pc_public_evals, vp_fri_query_digests ...), one after the other — [{kernel, workgroups, jobs, bytes, work, us}]."""
        n = lib_host().vph_verifier_launches(self.h, None, 0)
        arr = (LaunchStat * max(n, 1))()
        n = min(n, lib_host().vph_verifier_launches(self.h, arr, max(n, 1)))
        return [{"kernel": lib_gpu().vp_kernel_name(e.kind).decode(), "workgroups": e.workgroups, "jobs": e.jobs, "bytes": e.bytes, "work": e.work, "us": e.us}
                for e in arr[:max(n, 0)]]

    def pc_public_evals(self, leaf0, point=None, pub=None, n=None):
        """vp_pc_public_evals on the session's device: the public polynomials' values at the query points, (n_queries, 2, 64, 2) uint64 as
        Circuit.pc_public_evals_host.  point: (n, 2) uint64 (the vector is eq(point, .)) or pub: (2^n, 2); n defaults to the point's / the vector's size.
        Raises RuntimeError with the library's status and message on a refusal."""
        import numpy as np
        lf = np.ascontiguousarray(leaf0, dtype=np.uint64).reshape(-1)
        pt = None if point is None else np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 2)
        pb = None if pub is None else np.ascontiguousarray(pub, dtype=np.uint64).reshape(-1, 2)
        if n is None:
            n = pt.shape[0] if pt is not None else int(pb.shape[0]).bit_length() - 1
        out = np.zeros((max(len(lf), 1), 2, 64, 2), dtype=np.uint64)
        err = ctypes.create_string_buffer(512)
        rc = lib_host().vph_pc_public_evals(self.h, int(n), None if pt is None else pt.ctypes.data, None if pb is None else pb.ctypes.data, len(lf),
                                            lf.ctypes.data, out.ctypes.data, err, len(err))
        if rc:
            raise RuntimeError("vp_pc_public_evals failed: %d %s" % (rc, err.value.decode()))
        return out[: len(lf)]

    def pc_mask_evals(self, leaf0, pub_mask, ms, n=None):
        """vp_pc_mask_evals on the session's device: the public mask polynomial's values at the query points, (n_queries, 2, 2) uint64 as
        Circuit.pc_mask_evals_host; n defaults to the circuit's input bit length.  Raises RuntimeError with the library's status and message on a refusal."""
        import numpy as np
        if n is None:
            n = self.circuit.layer_bitlen(0)
        lf = np.ascontiguousarray(leaf0, dtype=np.uint64).reshape(-1)
        pm = np.ascontiguousarray(pub_mask, dtype=np.uint64).reshape(-1, 2)
        out = np.zeros((max(len(lf), 1), 2, 2), dtype=np.uint64)
        err = ctypes.create_string_buffer(512)
        rc = lib_host().vph_pc_mask_evals(self.h, int(n), pm.ctypes.data if pm.shape[0] else None, pm.shape[0], int(ms), len(lf), lf.ctypes.data, out.ctypes.data,
                                          err, len(err))
        if rc:
            raise RuntimeError("vp_pc_mask_evals failed: %d %s" % (rc, err.value.decode()))
        return out[: len(lf)]

    def fri_query_digests(self, leaf0, answer, n=None):
        """vp_fri_query_digests on the session's device: 64 bytes per opening of `answer` (vp_fri_query's layout for (n, len(leaf0)); n defaults to the
        circuit's input bit length) — recomputed leaf-chain digest | root reached through the path.  Raises RuntimeError on a refusal."""
        import numpy as np
        if n is None:
            n = self.circuit.layer_bitlen(0)
        lf = np.ascontiguousarray(leaf0, dtype=np.uint64).reshape(-1)
        buf = ctypes.create_string_buffer(bytes(answer), max(len(answer), 1))
        out = ctypes.create_string_buffer(max(len(lf) * max(n - 4, 0) * 64, 1))
        err = ctypes.create_string_buffer(512)
        rc = lib_host().vph_fri_query_digests(self.h, int(n), len(lf), lf.ctypes.data, ctypes.cast(buf, ctypes.c_void_p), len(answer),
                                              ctypes.cast(out, ctypes.c_void_p), err, len(err))
        if rc:
            raise RuntimeError("vp_fri_query_digests failed: %d %s" % (rc, err.value.decode()))
        return out.raw[: len(lf) * (n - 4) * 64]

    def last_full_record(self):
        """Record of the last accepted prove_and_verify_full() (layout: host/vphost.h): everything the prover handed over, for
        Circuit.verify_full_record — which needs no GPU."""
        n = ctypes.c_uint64(0)
        lib_host().vph_last_full_record(self.h, None, 0, ctypes.byref(n))
        if not n.value:
            raise RuntimeError("no accepted complete-protocol run on this session yet")
        buf = ctypes.create_string_buffer(n.value)
        if lib_host().vph_last_full_record(self.h, ctypes.cast(buf, ctypes.c_void_p), n.value, ctypes.byref(n)):
            raise RuntimeError("vph_last_full_record failed")
        return buf.raw[: n.value]

    def fri_open_many(self, requests, path_stride=OPEN_PATH_STRIDE):
        """vp_fri_open_many on this session's commitment: requests = sequence of (oracle, leaf); returns (values (n, 130, 2) uint64,
        paths (n, path_stride) uint8, path_len (n,) int32).  Raises on a refused list."""
        if self._shard_pc:                                  # asked of every rank and merged
            import numpy as np
            n = len(requests)
            oracle = np.ascontiguousarray([r[0] for r in requests], dtype=np.int32).reshape(n)
            leaf = np.ascontiguousarray([r[1] for r in requests], dtype=np.uint64).reshape(n)
            v = np.zeros((max(n, 1), 130, 2), dtype=np.uint64)
            p = np.zeros((max(n, 1), max(path_stride, 1)), dtype=np.uint8)
            pl = np.zeros(max(n, 1), dtype=np.int32)
            err = ctypes.create_string_buffer(512)
            if lib_host().vph_fri_open_many(self.h, n, oracle.ctypes.data, leaf.ctypes.data, v.ctypes.data, p.ctypes.data, path_stride, pl.ctypes.data, err, len(err)):
                raise RuntimeError("vp_fri_open_many failed: " + err.value.decode())
            return v[:n], p[:n], pl[:n]
        ctx = self.gpu_ctx()
        rc, v, p, pl = fri_open_many(ctx, requests, path_stride)
        if rc:
            raise RuntimeError("vp_fri_open_many failed: %d %s" % (rc, (lib_gpu().vp_last_error(ctx) or b"").decode()))
        return v, p, pl

    def fri_query(self, leaf0):
        """vp_fri_query: the complete answer to len(leaf0) query repetitions as bytes (layout: include/vpgpu.h)."""
        if self._shard_pc:                                  # every rank fills in the openings it owns
            import numpy as np
            leaf0 = np.ascontiguousarray(leaf0, dtype=np.uint64)
            n_bits = self.circuit.layer_bitlen(0)
            cap = leaf0.shape[0] * sum(2080 + 32 * d for d in [n_bits - 1, n_bits - 1] + [n_bits - 2 - k for k in range(n_bits - 6)])
            out = ctypes.create_string_buffer(max(cap, 1))
            n = ctypes.c_uint64(0)
            err = ctypes.create_string_buffer(512)
            if lib_host().vph_fri_query(self.h, leaf0.shape[0], leaf0.ctypes.data, ctypes.cast(out, ctypes.c_void_p), cap, ctypes.byref(n), err, len(err)):
                raise RuntimeError("vp_fri_query failed: " + err.value.decode())
            return out.raw[: n.value]
        ctx = self.gpu_ctx()
        rc, out = fri_query(ctx, leaf0)
        if rc:
            raise RuntimeError("vp_fri_query failed: %d %s" % (rc, (lib_gpu().vp_last_error(ctx) or b"").decode()))
        return out

    def last_fft_gkr(self):
        """Messages of fft_gkr (vp_fft_gkr layout) of the last prove_and_verify_full(), as bytes."""
        import numpy as np
        out = np.zeros((4096, 2), dtype=np.uint64)
        n = lib_host().vph_last_fft_gkr(self.h, out.ctypes.data, out.shape[0])
        if n < 0:
            raise RuntimeError("no complete-protocol run on this session yet")
        return out[:n].tobytes()

    def last_fri(self):
        """FRI commit phase of the last prove_and_verify_full(): (roots bytes, final codeword (2048, 2), challenges (steps, 2))."""
        import numpy as np
        roots = ctypes.create_string_buffer(32 * 32)
        fin = np.zeros((2048, 2), dtype=np.uint64)
        r = np.zeros((32, 2), dtype=np.uint64)
        st = lib_host().vph_last_fri(self.h, ctypes.cast(roots, ctypes.c_void_p), len(roots), fin.ctypes.data, r.ctypes.data)
        if st < 0:
            raise RuntimeError("no complete-protocol run on this session yet")
        return roots.raw[:32 * st], fin, r[:st].copy()

    def last_point(self):
        """r_liu after the last Liu sumcheck of the last prove_full / prove_and_verify_full, (n, 2) uint64."""
        import numpy as np
        out = np.zeros((64, 2), dtype=np.uint64)
        n = lib_host().vph_last_point(self.h, out.ctypes.data, 64)
        if n < 0:
            raise RuntimeError("no complete-protocol run on this session yet")
        return out[:n].copy()

    def eq_table(self, point):
        """eq(point, .) over 2^n entries on the device (vp_test_beta): the protocol's public vector for point = last_point()."""
        import numpy as np
        point = np.ascontiguousarray(point, dtype=np.uint64)
        n = point.shape[0]
        one = np.array([1, 0], dtype=np.uint64)
        out = np.zeros((1 << n, 2), dtype=np.uint64)
        rc = lib_gpu().vp_test_beta(lib_host().vph_session_ctx(self.h), point.ctypes.data, n, one.ctypes.data, out.ctypes.data)
        if rc:
            raise RuntimeError("vp_test_beta failed")
        return out

    def fri_commit(self, r, batched=True):
        """FRI commit phase with the given fold challenges ((steps, 2) uint64): (roots bytes, final codeword (2048, 2)).
        batched: all steps in one device pass (vp_fri_commit); otherwise one vp_fri_step per challenge."""
        import numpy as np
        r = np.ascontiguousarray(r, dtype=np.uint64)
        roots = ctypes.create_string_buffer(32 * r.shape[0])
        fin = np.zeros((2048, 2), dtype=np.uint64)
        err = ctypes.create_string_buffer(512)
        fn = lib_host().vph_fri_commit_batched if batched else lib_host().vph_fri_commit
        rc = fn(self.h, r.ctypes.data, r.shape[0], ctypes.cast(roots, ctypes.c_void_p), fin.ctypes.data, err, len(err))
        if rc:
            raise RuntimeError("fri_commit failed: " + err.value.decode())
        return roots.raw, fin

    def check(self, transcript, skip_predicates=False, device_predicates=False):
        """Replay the transcript through the host verifier: (accepted, seconds).  device_predicates: the O(|C|) wiring-predicate
        loops (verifier.cpp:50-113) run on the GPU (vp_predicates) instead of the host."""
        sec = ctypes.c_double(0)
        buf = ctypes.create_string_buffer(bytes(transcript), len(transcript))
        rc = lib_host().vph_check(self.h, ctypes.cast(buf, ctypes.c_void_p), len(transcript),
                                  (1 if skip_predicates else 0) | (2 if device_predicates else 0), ctypes.byref(sec))
        return rc == 0, sec.value

    def close(self):
        if self.h:
            lib_host().vph_session_free(self.h)
            self.h = None
