"""Builds tests/wavesim/build/libwavesim_kernels.so (build) and the libraries of the tests/sim_*_run.py drivers (build_sim); g++ only
(TEST INFRASTRUCTURE)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "build", "libwavesim_kernels.so")


def build(force=False, sanitize=False):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    srcs = [os.path.join(HERE, "sim_kernels.cpp"), os.path.join(HERE, "wavesim.cpp")]
    deps = srcs + [os.path.join(HERE, "wavesim.h")]
    csrc = os.path.join(HERE, "..", "..", "rust_compress_amd", "csrc")
    deps += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))]
    if not force and os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + (["-DRCX_SIM_TRACE"] if os.environ.get("RCX_SIM_TRACE") else []) + \
          (["-fsanitize=address", "-fno-omit-frame-pointer"] if (sanitize or os.environ.get("RCX_SIM_ASAN")) else []) + [ "-fPIC", "-shared", "-x", "c++", "-include", os.path.join(HERE, "wavesim.h"),
           "-Wall", "-DRCX_V8_WHY_STATS", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-unused-variable", "-Wno-attributes",
           "-o", OUT] + srcs
    subprocess.check_call(cmd)
    return OUT


def build_sim(out, src, kernel_files, extra_flags=()):
    """Builds the simulator library `out` of one tests/sim_*_run.py driver from `src` and wavesim.cpp, unless it is newer than all it is made
    of: src, the simulator, and kernel_files (names under rust_compress_amd/csrc that src includes).  The library is written under a
    temporary name and renamed: several test processes may build it at once.  -> out"""
    ws_h, ws_cpp = os.path.join(HERE, "wavesim.h"), os.path.join(HERE, "wavesim.cpp")
    csrc = os.path.join(HERE, "..", "..", "rust_compress_amd", "csrc")
    deps = [src, ws_h, ws_cpp] + [os.path.join(csrc, f) for f in kernel_files]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = out + ".%d" % os.getpid()
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-x", "c++", "-include", ws_h] + list(extra_flags) +
                          ["-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-unused-variable", "-Wno-attributes", "-o", tmp, src, ws_cpp])
    os.replace(tmp, out)
    return out


if __name__ == "__main__":
    print(build(force=True))
