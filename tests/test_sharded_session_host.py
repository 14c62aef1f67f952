"""CPU: the host library's entry for a session whose commitment is sharded over its ranks (host/vphost.h: vph_session_create_sharded).  No GPU is
needed: the symbols, and the refusal without a device."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

NEW = ("vph_session_create_sharded", "vph_commit_private_masked", "vph_commit_public_eq", "vph_fri_open_many", "vph_fri_query")


def test_sharded_session_entries_are_declared_and_exported(vp):
    hdr = open(os.path.join(ROOT, "virgo-plus_amd", "host", "vphost.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", vp.LIB_HOST], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r" T (vph_[a-z_0-9]+)", out))
    for s in NEW + ("vph_session_create_round_sharded",):
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in exported, s
        getattr(vp.lib_host(), s)
    # the device library's side: the owner query the host prover asks, declared for callers with a transport of their own
    gpu = subprocess.run(["nm", "-D", "--defined-only", vp.LIB_GPU], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert " T vp_pc_shard_owner" in gpu
    assert re.search(r"\bvp_pc_shard_owner\s*\(", open(os.path.join(ROOT, "include", "vpgpu.h")).read())


def test_sharded_session_needs_devices(vp):
    c = vp.Circuit.randomize(3, 8, seed=3)
    with pytest.raises(ValueError):
        vp.Session(c, shard_commitment=True)
    c.close()


def test_no_gpu_sharded_session_fails_with_a_message(vp):
    from conftest import gpu_count
    if gpu_count() > 0:
        pytest.skip("a GPU is present")
    c = vp.Circuit.randomize(3, 8, seed=3)
    err = ctypes.create_string_buffer(512)
    devs = (ctypes.c_int * 2)(0, 0)
    for shard in (0, 1):
        h = vp.lib_host().vph_session_create_sharded(c.h, devs, 2, 2, shard, None, err, len(err))
        assert not h and b"vp_create failed" in err.value
    assert not vp.lib_host().vph_session_create_sharded(None, devs, 2, 2, 1, None, err, len(err)) and err.value
    with pytest.raises(RuntimeError):
        vp.Session(c, devices=[0, 0], round_shard_min_log=2, shard_commitment=True)
    c.close()


def test_sanitizer_leg_builds_the_files_of_the_sharded_session():
    """tests/test_sanitizers.py lists its sources explicitly: the files that hold the new entry and the prover's rank loop are among them"""
    txt = open(os.path.join(ROOT, "tests", "test_sanitizers.py")).read()
    assert '"prover.cpp"' in txt and '"vphost.cpp"' in txt
    assert "vph_session_create_sharded" in open(os.path.join(ROOT, "virgo-plus_amd", "host", "vphost.cpp")).read()
