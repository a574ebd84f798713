"""csrc/decode_plan.h without a device: plan_decode() takes every launch decision of the Viterbi decode (workgroups, time slicing and its queues,
the back-pointer pool, the LDS layout, the instantiation), read_vit_env() reads the decoder's switches.  A small main, plain g++ -std=c++17, prints
the plan of each case; the expected values were derived by hand from the launch code this helper replaced.  Unless a case says otherwise:
streams 256, maxActive 65536, arenaTokens 0, U 1000, Tmax 998, nDist 1024, 50 000 states, static LDS 7 712 bytes, no switch set, and a device
that deals workgroups round robin over 8 XCDs.  The side records take 496 x 32 = 15 872 bytes of LDS, the state table 131 072."""
import os
import subprocess

import pytest

from tests.conftest import PKG

FIELDS = ("slots", "segFrames", "segQueues", "segCount", "arenaPer", "poolArenas", "useLdsRow", "hashN", "cntCap", "ldsBytes", "narrow", "modes", "rrCalls")
BASE = dict(slots=256, segFrames=125, segQueues=8, segCount=8, arenaPer=8192000, poolArenas=188, useLdsRow=1, hashN=16384, cntCap=2048,
            ldsBytes=155136, narrow=1, modes=4, rrCalls=1)
UNSLICED = dict(segFrames=0, segCount=1, poolArenas=0)         # run to completion: one "segment", no pool

# name -> (C++ statements that change the case's input `in`, switches `env` or round-robin answer `rr`; expected fields that differ from BASE)
CASES = {
    "base": ("", {}),
    "u256": ("in.U = 256;", dict(UNSLICED, rrCalls=0)),                                         # no more utterances than workgroups
    "states65535": ("in.nNodes = 65535;", {}),
    "states65536": ("in.nNodes = 65536;", dict(narrow=0, modes=0)),
    "table_wide": ("env.tableWide = true;", dict(narrow=0, modes=0)),
    "lattice": ("in.latticeTokens = 100000;", dict(UNSLICED, modes=6, rrCalls=0)),
    "tmax248": ("in.Tmax = 248;", dict(UNSLICED, arenaPer=8192 * 250, rrCalls=0)),             # 2 x 125 > 248 + 1
    "tmax249": ("in.Tmax = 249;", dict(segCount=2, arenaPer=8192 * 251, poolArenas=188)),
    "save_area": ("in.maxActive = 700000;", dict(UNSLICED, rrCalls=0)),                         # 1000 x 700 000 x 24 bytes = 16.8 GB > 16
    "not_round_robin": ("rr = false;", dict(UNSLICED)),
    "streams60": ("in.streams = 60; in.U = 100;", dict(UNSLICED, slots=60, rrCalls=0)),         # the device is not asked
    "streams60_any": ("in.streams = 60; in.U = 100; env.segAny = 1;", dict(slots=60, segQueues=1, poolArenas=19, rrCalls=0)),
    "seg_any2": ("env.segAny = 2;", dict(segQueues=1)),
    "ndist2296": ("in.nDist = 2296;", dict(cntCap=0, ldsBytes=156128)),                        # 9 184 + 131 072 + 15 872 = 160 KB - 7 712 exactly
    "ndist2297": ("in.nDist = 2297;", dict(useLdsRow=0, ldsBytes=151056)),                     # row in memory: 16 + 131 072 + 15 872 + 4 096
    "prof2204": ("env.prof = true; in.staticLds = 8080; in.nDist = 2204;", dict(cntCap=0, ldsBytes=155760, modes=5)),
    "prof2296": ("env.prof = true; in.staticLds = 8080; in.nDist = 2296;", dict(useLdsRow=0, ldsBytes=151056, modes=5)),
    "nohash": ("env.noHash = true;", dict(hashN=0, cntCap=0, ldsBytes=4096 + 15872, narrow=0, modes=0)),
    "nocnt": ("env.noCnt = true;", dict(cntCap=0, ldsBytes=151040)),
    "dump": ("in.dumpOn = true;", dict(UNSLICED, slots=1, modes=6, rrCalls=0)),
}

MAIN = r"""
#include "decode_plan.h"
#include <cstdio>
#include <cstring>
using namespace dsr;
static void show(const char* name, const PlanIn& in, const VitEnv& env, bool rr)
{
  int calls = 0;
  const DecodePlan p = plan_decode(in, env, [&] { calls++; return rr; });
  printf("%s %d %d %d %d %ld %d %d %d %d %zu %d %d %d\n", name, p.slots, p.segFrames, p.segQueues, p.segCount, p.arenaPer, p.poolArenas, p.useLdsRow, p.hashN,
         p.cntCap, p.ldsBytes, (int) p.narrow, p.modes, calls);
}
int main(int argc, char** argv)
{
  if (argc > 1 && !strcmp(argv[1], "env")) {
    const VitEnv e = read_vit_env();
    printf("%d %d %d %g %d %d %d %d %d %d %d %d\n", e.slots, (int) e.noFast, e.seg, e.segSaveGB, e.segAny, e.segDrop, (int) e.segVerbose, (int) e.pen, (int) e.prof,
           (int) e.noHash, (int) e.noCnt, (int) e.tableWide);
    return 0;
  }
  PlanIn base; base.streams = 256; base.maxActive = 65536; base.arenaTokens = 0; base.latticeTokens = 0; base.topN = 0; base.dumpOn = false;
  base.nNodes = 50000; base.maxCnt = 100; base.U = 1000; base.Tmax = 998; base.nDist = 1024; base.staticLds = 7712;
@CASES@  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    body = "".join('  { PlanIn in = base; VitEnv env; bool rr = true; %s show("%s", in, env, rr); }\n' % (code, name) for name, (code, _) in CASES.items())
    (d / "p.cpp").write_text(MAIN.replace("@CASES@", body))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(PKG, "csrc"), str(d / "p.cpp"), "-o", str(d / "p")])
    return str(d / "p")


@pytest.fixture(scope="module")
def plans(exe):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DSR_VITERBI_")}
    out = subprocess.run([exe], capture_output=True, text=True, env=env, check=True).stdout
    return {l.split()[0]: dict(zip(FIELDS, map(int, l.split()[1:]))) for l in out.strip().split("\n")}


@pytest.mark.parametrize("name", list(CASES))
def test_plan(plans, name):
    want = dict(BASE, **CASES[name][1])
    for f in FIELDS:
        assert plans[name][f] == want[f], (name, f, plans[name], want)


def test_read_vit_env(exe):
    """read_vit_env(): the defaults, and each DSR_VITERBI_* switch as the launch code parsed it."""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("DSR_VITERBI_")}
    run = lambda extra: subprocess.run([exe, "env"], capture_output=True, text=True, env=dict(clean, **extra), check=True).stdout.split()
    assert run({}) == ["0", "0", "125", "16", "0", "0", "0", "0", "0", "0", "0", "0"]
    sw = {"SLOTS": "64", "NOFAST": "1", "SEG": "50", "SEG_SAVE_GB": "2.5", "SEG_ANY": "2", "SEG_DROP": "0x81", "SEG_VERBOSE": "1", "PEN": "1", "PROF": "1",
          "NOHASH": "1", "NOCNT": "1", "TABLE": "wide"}
    assert run({"DSR_VITERBI_" + k: v for k, v in sw.items()}) == ["64", "1", "50", "2.5", "2", "129", "1", "1", "1", "1", "1", "1"]
    other = run({"DSR_VITERBI_SEG": "0", "DSR_VITERBI_SEG_ANY": "1", "DSR_VITERBI_TABLE": "narrow"})
    assert (other[2], other[4], other[11]) == ("0", "1", "0")
