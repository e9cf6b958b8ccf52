"""Several engines on one device at the same time, one host thread each, against the oracle.

A benchmarked serving mode (bench.py --full: C2+C3_inflight, C2_batch2, C3_batch2) that runs code
no single-threaded test reaches: the `shared` packing rule of the Part-1 decoder (taken only while
another engine of the device is inside a call; gk_timings::t1_shared says that it was), HostPool::run
finding the pool taken and running its items inline, the pinned page pool and the busy counts shared
by the engines of a process, and the launchers' first calls made by two threads together.

Every scenario (tests/inflight_cases.py) runs in a child process of its own: the launchers' statics
are initialised once per process, so only a fresh process lets two threads make the first call
together; a deadlock ends at the child's time limit; and GK_PCRD_CHUNK is read once per process.
The oracle judges every result.  The children print what they observed (the share of decodes that ran
under the shared rule, per case, and the occupiers' size), which `pytest -s` shows.
"""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CODE = r'''
import sys
sys.path[:0] = [%r, %r, %r]
import inflight_cases
inflight_cases.main(*sys.argv[1:])
''' % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))


def _child(*args, env=None):
    r = subprocess.run([sys.executable, "-c", CODE] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=240, env=dict(os.environ, **(env or {})))
    print(r.stdout, end="")
    assert r.returncode == 0 and "\nok " in "\n" + r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("pairing", ["decode_decode", "encode_decode", "ht_part1", "97_layers_53"])
def test_first_calls_together(pairing):
    # two threads' first calls in the process, released by a barrier
    _child("cold", pairing)


@pytest.mark.parametrize("nthreads", [2, 3, 4])
def test_mixed_work(nthreads):
    # every thread walks one list of encodes and decodes of every kind, rotated by its index
    _child("mixed", nthreads)


def test_settings_stay_with_their_engine():
    # one engine holds reduce 1 and one layer, one the display flag; two others decode plainly
    _child("sticky")


def test_host_pool_contended():
    # rate-controlled encodes of 1089 blocks (more than one PCRD chunk of 512), two threads, then three
    _child("pool", "chunk512")


def test_host_pool_many_short_jobs():
    # chunks of 16 blocks and tiles: pooled and inline execution alternate between the threads; one
    # case by quality, and refused encodes while the other threads' valid ones are in progress
    _child("pool", "chunk16", env={"GK_PCRD_CHUNK": "16"})


def test_shared_packing_rule():
    # every case of the matrix observed under the shared rule (t1_shared >= 1) within 20 decodes, with
    # the split it is built to produce, while two occupiers loop an encode each; samples equal the
    # oracle's in every decode, shared or not
    out = _child("shared")
    assert out.count("\nshared ") + out.startswith("shared ") == 9, out


def test_engines_created_and_destroyed_beside_running_ones():
    _child("churn")
