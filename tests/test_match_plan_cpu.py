"""The matcher's batch plan, checked on the host: tests/host/match_plan_check.cc runs plan_batch (and the other pure
host decisions of orthosfm_amd/csrc/match_plan.hip) over the sizes and modes at which the plan changes path, under
AddressSanitizer and UBSan, and checks what the kernels rely on: every range a problem owns in a scratch array lies
inside the plan's totals and apart from every other, block counts add up, segment lengths and kernel forms follow
their rules, every special-row entry has its jobs once per chunk."""
import os
import re
import subprocess


def test_batch_plan_invariants_hold_on_the_host():
    exe = os.path.join(os.path.dirname(__file__), "host", "match_plan_check")
    assert os.path.exists(exe), "tests/host/match_plan_check missing: run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1]
    m = re.fullmatch(r"ok (\d+) cases", last)
    assert m, r.stdout + r.stderr
    assert int(m.group(1)) > 10000, last
