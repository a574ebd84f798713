"""The host half of the kernel units without a device.  csrc/value_list.h: ints<...> states the values a template is instantiated for once,
has_value asks whether a run-time value is one of them, for_value hands the matching one to a callback as a compile-time constant (a small main,
plain g++ -std=c++17, prints what the callback saw).  csrc/launch.h: the only file of csrc/ that launches a kernel or raises a kernel's dynamic-LDS
limit, and no macro wraps it.  The beamformer family's kernel units (k_sph, k_beamform, k_mmi), the filter bank's (k_filterbank) and the
localization family's (k_doa, k_gcc, k_mcc, k_tracker) hold no C entries, and no file restates another unit's declaration by hand.  Timing events are
created by the two helpers of csrc/common.h."""
import glob
import os
import re
import subprocess

import pytest

from tests.conftest import PKG

CSRC = os.path.join(PKG, "csrc")
LISTED = (0, 4, 6, 8)
PROBES = LISTED + (5, -1)

MAIN = r"""
#include "value_list.h"
#include <cstdio>
using namespace dsr;
using L = ints<0, 4, 6, 8>;
static_assert(has_value(L{}, 6) && !has_value(L{}, 5), "has_value is usable at compile time");
template <int V> struct Tag { static constexpr int value = V; };
int main()
{
  const int probes[] = {@PROBES@};
  for (int v : probes) {
    int calls = 0, seen = -99, asTemplateArg = -99;
    const bool found = for_value(L{}, v, [&](auto c) { calls++; seen = c; asTemplateArg = Tag<c()>::value; });
    printf("%d %d %d %d %d %d\n", v, (int) found, calls, seen, asTemplateArg, (int) has_value(L{}, v));
  }
  int calls = 0;
  const bool twice = for_value(ints<3, 3>{}, 3, [&](auto) { calls++; });               // a value listed twice: the fold stops at the first match
  const bool none = for_value(ints<>{}, 3, [&](auto) { calls += 100; });
  printf("dup %d %d %d %d\n", (int) twice, calls, (int) none, (int) has_value(ints<>{}, 3));
  return 0;
}
"""


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("value_list")
    (d / "v.cpp").write_text(MAIN.replace("@PROBES@", ", ".join(map(str, PROBES))))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(d / "v.cpp"), "-o", str(d / "v")])
    out = subprocess.run([str(d / "v")], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    return {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out}


@pytest.mark.parametrize("v", LISTED)
def test_for_value_calls_once_with_the_listed_value(lines, v):
    found, calls, seen, as_template_arg, has = lines[str(v)]
    assert (found, calls, seen, as_template_arg, has) == (1, 1, v, v, 1)


@pytest.mark.parametrize("v", (5, -1))
def test_for_value_runs_nothing_for_a_value_not_listed(lines, v):
    found, calls, seen, as_template_arg, has = lines[str(v)]
    assert (found, calls, seen, as_template_arg, has) == (0, 0, -99, -99, 0)


def test_for_value_runs_at_most_once_and_never_for_an_empty_list(lines):
    assert lines["dup"] == [1, 1, 0, 0]


def _sources():
    files = sorted(f for pat in ("*.hip", "*.cpp", "*.h") for f in glob.glob(os.path.join(CSRC, pat)))
    assert len(files) > 60 and os.path.join(CSRC, "launch.h") in files
    return files


def test_kernels_are_launched_in_launch_h_only():
    hits = {}
    for f in _sources():
        text = open(f).read()
        for s in ("hipLaunchKernelGGL", "<<<", "hipFuncSetAttribute"):
            if s in text:
                hits.setdefault(s, []).append(os.path.basename(f))
    assert hits == {"hipLaunchKernelGGL": ["launch.h"], "hipFuncSetAttribute": ["launch.h"]}
    kernel_units = [f for f in _sources() if os.path.basename(f).startswith("k_") and f.endswith(".hip")]
    assert len(kernel_units) == 32
    assert [os.path.basename(f) for f in kernel_units if not re.search(r"\blaunch(_n)?\(", open(f).read())] == []


def test_split_kernel_units_hold_no_entries_and_no_unit_restates_a_declaration():
    for name in ("k_sph.hip", "k_beamform.hip", "k_mmi.hip", "k_filterbank.hip", "k_doa.hip", "k_gcc.hip", "k_mcc.hip", "k_tracker.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert [s for s in ('extern "C"', "dsr_status") if s in text] == [], name
    restated = re.compile(r'^namespace dsr \{ .*\); *\}|extern "C" \{ namespace dsr \{')   # a one-line declaration of another unit's function
    bad = []
    for f in _sources():
        bad += [(os.path.basename(f), n + 1) for n, l in enumerate(open(f).read().split("\n")) if restated.search(l)]
    assert bad == []


def test_timing_events_are_created_in_common_h():
    # k_lpc.hip and k_train.hip create their events per call; capi.cpp and decoder.cpp hold the pipe's and the decoder's own
    hits = sorted(os.path.basename(f) for f in _sources() if "hipEventCreate" in open(f).read())
    assert hits == ["capi.cpp", "common.h", "decoder.cpp", "k_lpc.hip", "k_train.hip"]


def test_no_macro_wraps_launch():
    bad = []
    for f in _sources():
        text = open(f).read().replace("\\\n", " ")                 # a continued #define is one logical line
        bad += [(os.path.basename(f), l.split()[1]) for l in text.split("\n") if re.match(r"\s*#\s*define\b", l) and "launch(" in l]
    assert bad == []
