"""CPU test of csrc/sr_dispatch.h: the width bucket and the two pickers that take a launcher from a run-time value to a
template instantiation, compiled alone (no HIP) into a stand-alone host program."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

MAIN = r"""
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include "sr_dispatch.h"

static char g_err[256];
void sr_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }

static int g_fail = 0;
#define EXPECT(...) do { if (!(__VA_ARGS__)) { std::printf("line %d: %s\n", __LINE__, #__VA_ARGS__); ++g_fail; } } while (0)

static_assert(sr_width_bucket(1) == 3 && sr_width_bucket(12) == 12, "constexpr");

int main() {
    const int bucket[12] = {3, 3, 3, 5, 5, 8, 8, 8, 12, 12, 12, 12};
    for (int D = 1; D <= 12; ++D) {
        EXPECT(sr_width_bucket(D) == bucket[D - 1]);
        // called exactly once, with the bucket as the constant; the functor's return code comes back unchanged
        int calls = 0, got = 0;
        const int rc = sr_pick_le<3, 5, 8, 12>("t", D, [&](auto w) { ++calls; got = decltype(w)::value; return 1000 + D; });
        EXPECT(calls == 1 && got == bucket[D - 1] && rc == 1000 + D);
    }
    for (int rc_in : {SR_OK, SR_EHIP, SR_EINVAL, 7})
        EXPECT(sr_pick_le<3, 5, 8, 12>("t", 4, [&](auto) { return rc_in; }) == rc_in);
    {   // beyond the widest: refused, the functor is not called
        int calls = 0;
        g_err[0] = 0;
        EXPECT(sr_pick_le<3, 5, 8, 12>("predict_grad", 13, [&](auto) { ++calls; return SR_OK; }) == SR_EUNSUPPORTED);
        EXPECT(calls == 0 && std::strcmp(g_err, "predict_grad: D=13 > 12") == 0);
        EXPECT(sr_pick_le<3, 5, 8>("w", 9, [&](auto) { ++calls; return SR_OK; }) == SR_EUNSUPPORTED);      // a site's own list
        EXPECT(calls == 0 && std::strcmp(g_err, "w: D=9 > 8") == 0);
    }
    for (int Np : {128, 256, 384, 512}) {
        int calls = 0, got = 0;
        g_err[0] = 0;
        EXPECT(sr_pick_eq<128, 256, 384, 512>("Np=%d not supported", Np, [&](auto n) { ++calls; got = decltype(n)::value; return 5; }) == 5);
        EXPECT(calls == 1 && got == Np && g_err[0] == 0);
        EXPECT(sr_pick_np("Np=%d not supported", Np, [&](auto n) { return (int)decltype(n)::value; }) == Np);
    }
    for (int Np : {640, 0, 127, 129, 200}) {
        int calls = 0;
        g_err[0] = 0;
        EXPECT(sr_pick_eq<128, 256, 384, 512>("t: Np=%d not supported", Np, [&](auto) { ++calls; return SR_OK; }) == SR_EUNSUPPORTED);
        char want[64];
        std::snprintf(want, sizeof want, "t: Np=%d not supported", Np);
        EXPECT(calls == 0 && std::strcmp(g_err, want) == 0);
        EXPECT(sr_pick_np("t: Np=%d not supported", Np, [&](auto) { ++calls; return SR_OK; }) == SR_EUNSUPPORTED && calls == 0);
    }
    if (g_fail) std::printf("FAILED %d\n", g_fail);
    else std::printf("dispatch OK\n");
    return g_fail ? 1 : 0;
}
"""


def test_dispatch_helpers_in_a_host_program(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "dispatch_main.cpp"
    src.write_text(MAIN)
    exe = str(tmp_path / "dispatch_main")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "safe_exploration_amd", "csrc"),
                         str(src), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "dispatch OK" in run.stdout, run.stdout + run.stderr
