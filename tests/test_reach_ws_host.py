"""CPU test of csrc/sr_reach_ws.h: the one layout of the handle's reach_ws, compiled alone (no HIP) into a stand-alone host
program.  The sizes below are written out from the table of blocks (doubles per row), not taken from the header:

   #      block                                size                       one step   roll-out 0   roll-out 1      roll-out 2
   1      z                                    D                          yes        yes          yes             yes
   2, 3   mu, var                              n_s each                   yes        yes          yes             yes
   4, 5   jac_mu, jac_var                      n_s D each                 yes        yes          yes             yes
   6      hess_mu                              n_s D^2                    yes        yes          if `second`     no
   7, 8   mu_bar, var_bar                      n_s each                   yes        yes          yes             yes
   9, 10  jac_bar, jac_s                       n_s (n_s + n_u) each       yes        yes          yes             no
   11     jz                                   n_s D                      yes        yes          yes             no
   12-15  q_in, kfb_in, p_seed, q_seed         n_s^2, n_u n_s, n_s, n_s^2 no         yes          yes             yes
   16-19  p_bar, q_bar, kff_bar, kfb_bar       n_s, n_s^2, n_u, n_u n_s   no         yes          yes             yes
   20     eig                                  1 + 2 n_s + n_u            no         yes          no              no
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

MAIN = r"""
#include <cstdio>
#include <vector>
#include "sr_reach_ws.h"

static int g_fail = 0;
#define EXPECT(...) do { if (!(__VA_ARGS__)) { if (g_fail < 20) std::printf("line %d (n_s=%d n_u=%d D=%d rollout=%d mode=%d second=%d rows=%ld): %s\n", \
    __LINE__, n_s, n_u, D, (int)rollout, mode, (int)second, rows, #__VA_ARGS__); ++g_fail; } } while (0)

int main() {
    long cases = 0;
    for (int n_s = 1; n_s <= 8; ++n_s)
    for (int n_u = 1; n_u <= 4; ++n_u)
    for (int D = 2; D <= 8; ++D)
    for (int rollout = 0; rollout <= 1; ++rollout)
    for (int mode = 0; mode <= 2; ++mode)
    for (int second = 0; second <= 1; ++second)
    for (long rows : {1L, 21L, 63L}) {
        // the table's column of this configuration, block by block
        const bool hess = !rollout || mode == 0 || (mode == 1 && second);
        const bool link = !rollout || mode != 2;
        const bool eig = rollout && mode == 0;
        const long nss = (long)n_s * n_s, nus = (long)n_u * n_s, nd = (long)n_s * D, nds = (long)n_s * (n_s + n_u);
        const long size[20] = {D, n_s, n_s, nd, nd, hess ? nd * D : -1, n_s, n_s, link ? nds : -1, link ? nds : -1, link ? nd : -1,
                               rollout ? nss : -1, rollout ? nus : -1, rollout ? n_s : -1, rollout ? nss : -1,
                               rollout ? n_s : -1, rollout ? nss : -1, rollout ? n_u : -1, rollout ? nus : -1,
                               eig ? 1 + 2 * n_s + n_u : -1};
        long total = D + 4L * n_s + 2 * nd;                                              // blocks 1 - 5, 7, 8
        if (hess) total += nd * D;
        if (link) total += 2 * nds + nd;
        if (rollout) total += 3 * nss + 2 * nus + 2L * n_s + n_u;
        if (eig) total += 1 + 2L * n_s + n_u;

        const sr_reach_ws_use use{n_s, n_u, D, rollout != 0, mode, second != 0};
        const sr_reach_ws dry = sr_reach_ws_carve(use, rows, nullptr);
        EXPECT(dry.per == total);
        std::vector<double> buf((size_t)(rows * total) + 1);
        const sr_reach_ws w = sr_reach_ws_carve(use, rows, buf.data());
        EXPECT(w.per == dry.per);
        double* const got[20] = {w.z, w.mu, w.var, w.jac_mu, w.jac_var, w.hess_mu, w.mu_bar, w.var_bar, w.jac_bar, w.jac_s, w.jz,
                                 w.q_in, w.kfb_in, w.p_seed, w.q_seed, w.p_bar, w.q_bar, w.kff_bar, w.kfb_bar, w.eig};
        double* const dry_got[20] = {dry.z, dry.mu, dry.var, dry.jac_mu, dry.jac_var, dry.hess_mu, dry.mu_bar, dry.var_bar,
                                     dry.jac_bar, dry.jac_s, dry.jz, dry.q_in, dry.kfb_in, dry.p_seed, dry.q_seed, dry.p_bar,
                                     dry.q_bar, dry.kff_bar, dry.kfb_bar, dry.eig};
        double* next = buf.data();
        for (int k = 0; k < 20; ++k) {
            EXPECT(dry_got[k] == nullptr);
            if (size[k] < 0) { EXPECT(got[k] == nullptr); continue; }
            EXPECT(got[k] == next);                                                      // starts where the previous block ends
            if (got[k] == next) { got[k][0] = 1.0; got[k][rows * size[k] - 1] = 2.0; }   // (in bounds: the sanitizer's say)
            next += rows * size[k];
        }
        EXPECT(next == buf.data() + rows * total);                                       // the last block ends at the total
        ++cases;
    }
    if (g_fail) std::printf("FAILED %d\n", g_fail);
    else std::printf("reach_ws OK %ld\n", cases);
    return g_fail ? 1 : 0;
}
"""


def test_reach_ws_layout_in_a_host_program(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "reach_ws_main.cpp"
    src.write_text(MAIN)
    exe = str(tmp_path / "reach_ws_main")
    base = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "safe_exploration_amd", "csrc"), str(src),
            "-o", exe]
    # with the address and undefined-behaviour sanitizers where this compiler builds an empty program with them that runs
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probe_exe = str(tmp_path / "probe")
    ok = subprocess.run([cxx, str(probe), "-o", probe_exe] + san, capture_output=True).returncode == 0 and \
        subprocess.run([probe_exe], capture_output=True).returncode == 0
    cc = subprocess.run(base + (san if ok else []), capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "reach_ws OK %d" % (8 * 4 * 7 * 2 * 3 * 2 * 3) in run.stdout, run.stdout + run.stderr
