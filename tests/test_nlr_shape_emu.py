"""CPU: the grid and split arithmetic of the z stages that end in a reduction (csrc/nlr_shape.h), which the loop over the rows of a
batch (csrc/core.hip nlr_rows) follows -- emulator group `nlrshape`, no device and nothing allocated.  For resident-workgroup caps
1, 7 and 1024, tiles 1, 4 and 16, rows of 64, 4096 and 65535 points and row counts from 1 up to more than five launches' worth
(2^32 values per workgroup are plain integers on the host), per combination: successive launches cover every row exactly once;
each launch of a kind that counts keeps passes * 2 * tile * n below 2^32, passes = ceil(units / ngroups); 1 <= ngroups <=
min(units, cap); a kind that sums doubles makes exactly one launch."""
import re

from emu_util import run_group


def test_split_arithmetic():
    r = run_group("nlrshape")
    assert r.returncode == 0 and "EMU TESTS PASSED" in r.stdout, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("nlr_shape cap=")]
    seen = set()
    for l in lines:
        m = re.match(r"nlr_shape cap=(\d+) tile=(\d+)\s+N=(\d+)\s", l)
        assert m and l.rstrip().endswith("ok"), l
        seen.add(tuple(int(x) for x in m.groups()))
    assert seen == {(c, t, n) for c in (1, 7, 1024) for t in (1, 4, 16) for n in (64, 4096, 65535)}, sorted(seen)
    refused = [l for l in r.stdout.splitlines() if l.startswith("nlr_shape pass too long")]
    assert len(refused) == 1 and refused[0].rstrip().endswith("ok"), refused
