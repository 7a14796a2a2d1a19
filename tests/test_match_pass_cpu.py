"""The passes of a batch over the device, checked on the host: tests/host/match_pass_check.cc runs the slice bounds of the
post-work (1 to 70 pairs against 1 to 9 requested slices, the default, the knob's extremes) and the layouts of the
control, staging and compaction blocks (1, 2, 407 and 4096 problems, with and without SURF problems, rescore buckets and
special jobs) under AddressSanitizer and UBSan: slices tile the pairs in order with none empty, every field lies inside
its block, aligned and apart from the others."""
import os
import re
import subprocess


def test_slice_bounds_and_block_layouts_hold_on_the_host():
    exe = os.path.join(os.path.dirname(__file__), "host", "match_pass_check")
    assert os.path.exists(exe), "tests/host/match_pass_check missing: run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1]
    m = re.fullmatch(r"ok (\d+) cases", last)
    assert m, r.stdout + r.stderr
    assert int(m.group(1)) >= 70 * 9 + 4 * 2, last
