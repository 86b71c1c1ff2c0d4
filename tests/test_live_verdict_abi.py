"""The live verdict and G.711 push entry points (tfp_live_verdict, tfp_live_push_g711 and the group's):
exported, declared and bound; struct tfp_live_verdict's size and field offsets in the ctypes mirror
equal a compiled C probe's; the argument rules that need no device; and the rule itself
(csrc/tfp_live_plan.hpp, live_verdict_rule) against its statement in the header. No GPU."""
import ctypes as C
import os
import subprocess

from conftest import REPO

NEW_SYMBOLS = ["tfp_live_verdict", "tfp_live_push_g711", "tfp_group_live_verdict", "tfp_group_live_push_g711"]
FIELDS = ["leader", "rival", "has_leader", "has_rival", "remaining", "complete", "decided"]
TFP_E_ARG = -1

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "tiresias_fp.h"
int main(void) {
  printf("%zu", sizeof(struct tfp_live_verdict));
OFFSETS
  printf("\n");
  return 0;
}
"""


def test_symbols_exported_declared_and_bound(tfp_lib):
    from tiresias_amd import _lib
    syms = _lib.header_symbols()
    lib = tfp_lib.lib()
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in _lib._SIGS, name
        assert hasattr(lib, name), name
    for cls in (tfp_lib.Live, tfp_lib.GroupLive):
        for m in ("push_g711", "verdict"):
            assert callable(getattr(cls, m))


def test_struct_layout_matches_a_c_probe(tfp_lib, tmp_path):
    from tiresias_amd._lib import LiveVerdict
    src = tmp_path / "probe.c"
    src.write_text(PROBE.replace("OFFSETS", "\n".join('  printf(" %%zu", offsetof(struct tfp_live_verdict, %s));' % f for f in FIELDS)))
    exe = str(tmp_path / "probe")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(LiveVerdict)
    assert got[1:] == [getattr(LiveVerdict, f).offset for f in FIELDS]
    assert [n for n, _ in LiveVerdict._fields_] == FIELDS


def test_argument_rules_that_need_no_device(tfp_lib):
    lib = tfp_lib.lib()
    assert lib.tfp_live_verdict(None, None, None, None, None) == TFP_E_ARG
    assert lib.tfp_group_live_verdict(None, None, None, None, None) == TFP_E_ARG
    assert lib.tfp_live_push_g711(None, None, 160, 0, None, None, None, 1, None, None, None) == TFP_E_ARG
    assert lib.tfp_group_live_push_g711(None, None, 160, 0, None, None, None, 1, None, None, None) == TFP_E_ARG


RULE = r"""
#include <stdio.h>
#include "tfp_live_plan.hpp"
using namespace tfp;
static unsigned long long key(unsigned long long count, unsigned long long tie) { return ((count << 32) | tie) + 1; }
int main() {
  // S = 2080 of 4096: 8 final frames, 8 to come
  const int64_t S = 2080, total = 4096;
  int bad = 0;
  LiveVerdictRule r = live_verdict_rule(key(8, 3), key(0, 5), S, total);  // count == remaining, the rival's key greater
  bad |= !(r.has_leader && r.has_rival && r.remaining == 8 && !r.complete && !r.decided);
  r = live_verdict_rule(key(8, 5), key(0, 3), S, total);  // ... the leader's key greater: the strict comparison holds
  bad |= !(r.decided && (r.rival >> 32) == 0 && (r.rival & 0xffffffffull) == 3) << 1;
  r = live_verdict_rule(key(9, 3), key(0, 5), S + 256, total);  // one frame later
  bad |= !(r.decided && r.remaining == 7) << 2;
  r = live_verdict_rule(key(0, 9), key(0, 5), S, total);  // the greatest candidate has count 0: no leader, no rival
  bad |= !(!r.has_leader && !r.has_rival && !r.decided) << 3;
  r = live_verdict_rule(key(1, 0), 0, 256, total);  // a single candidate: decided from the first hit
  bad |= !(r.has_leader && !r.has_rival && r.decided) << 4;
  r = live_verdict_rule(0, 0, total, total);  // complete: decided, leader or not
  bad |= !(r.complete && r.decided && r.remaining == 0) << 5;
  r = live_verdict_rule(key(65535, 2147483647ull), key(65535, 0), S, total);  // the keys' edges: the + 1 stays in the low word
  bad |= !((r.leader >> 32) == 65535 && (r.leader & 0xffffffffull) == 2147483647ull && !r.decided) << 6;
  r = live_verdict_rule(key(3, 1), key(3, 0), 255, 255);  // S == total with a tail only
  bad |= !(r.complete && r.remaining == 0 && r.decided) << 7;
  r = live_verdict_rule(key(1, 1), key(0, 0), 255, 257);  // no final frame yet, two to come
  bad |= !(r.remaining == 2 && !r.decided) << 8;
  printf("%d\n", bad);
  return bad != 0;
}
"""


def test_rule_asan_ubsan(tmp_path):
    src = tmp_path / "rule.cpp"
    src.write_text(RULE)
    exe = str(tmp_path / "rule")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1",
                    "-I" + os.path.join(REPO, "asterisk-tiresias_amd", "csrc"), str(src), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "0", (r.stdout, r.stderr[-2000:])
