"""``csrc/field_dealing.h`` on the host: which wave of the fused field kernels visits which 16-point group, and how many
workgroups the host launches.  The header is plain integer arithmetic, so a C++ program enumerates every
(grid, block, wave) and checks the cover; no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_MAIN = r"""
#include <stdio.h>
#include <vector>
#include "field_dealing.h"

int main()
{
    const int waves = 8;
    const unsigned grids[] = {1, 5, 8, 63, 64, 72, 256};
    std::vector<long> sizes;
    for (long n = 1; n <= 600; ++n) sizes.push_back(n);
    sizes.push_back(4095); sizes.push_back(4096); sizes.push_back(4097);
    long bad_cover = 0, bad_eighth = 0, cases = 0;
    for (long n : sizes)
        for (unsigned grid : grids) {
            std::vector<int> seen(n, 0);
            const long per_xcd = (n + 7) / 8;
            for (unsigned b = 0; b < grid; ++b)
                for (int w = 0; w < waves; ++w) {
                    const QfGroupRange r = qf_group_range(n, grid, b, w, waves);
                    if (r.stride <= 0) { ++bad_cover; continue; }
                    for (int64_t g = r.begin; g < r.end; g += r.stride) {
                        if (g < 0 || g >= n) { ++bad_cover; continue; }
                        ++seen[g];
                        if (grid % 8 == 0 && g / per_xcd != (long)(b & 7)) ++bad_eighth;
                    }
                }
            for (long g = 0; g < n; ++g) bad_cover += seen[g] != 1;
            ++cases;
        }
    long bad_blocks = 0;
    const int cus[] = {1, 64, 256, 304};
    for (long n : sizes)
        for (int cu : cus) {
            const int64_t blocks = qf_field_blocks(n, waves, cu);
            if (blocks < 1 || blocks > cu || (blocks >= 64 && blocks % 8 != 0)) ++bad_blocks;
        }
    // the sizes the GPU tests rely on: 8197 points take the XCD route on a 256-CU part, 4101 and 4096 the other one
    printf("cases %ld\nbad_cover %ld\nbad_eighth %ld\nbad_blocks %ld\n", cases, bad_cover, bad_eighth, bad_blocks);
    printf("blocks_513 %ld\nblocks_257 %ld\nblocks_256 %ld\n", (long)qf_field_blocks(513, waves, 256),
           (long)qf_field_blocks(257, waves, 256), (long)qf_field_blocks(256, waves, 256));
    printf("clamp %ld %ld %ld\n", (long)qf_clamp_count(-3, 10), (long)qf_clamp_count(7, 10), (long)qf_clamp_count(11, 10));
    return 0;
}
"""


def test_every_group_is_dealt_once_and_blocks_follow_the_rule(tmp_path):
    """n_groups 1..600 and 4095..4097 on grids {1, 5, 8, 63, 64, 72, 256} of 8-wave workgroups: every group is visited
    exactly once; on a grid that is a multiple of 8, workgroup b only sees groups of eighth b & 7.  qf_field_blocks is
    >= 1, <= the CU count and a multiple of 8 from 64 on, for 1, 64, 256 and 304 CUs."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "dealing.cpp"
    src.write_text(_MAIN)
    exe = tmp_path / "dealing"
    inc = os.path.join(ROOT, "quadraturefields_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", inc, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in out.splitlines() if l.strip()}
    assert got["cases"] == [603 * 7]
    assert got["bad_cover"] == [0]
    assert got["bad_eighth"] == [0]
    assert got["bad_blocks"] == [0]
    assert got["blocks_513"] == [64] and got["blocks_257"] == [33] and got["blocks_256"] == [32]
    assert got["clamp"] == [0, 7, 10]
