"""Counts the most steps the series and the two continued fractions of csrc/dist_math.hpp take over the domain
(0 < df <= 1e4): the figures next to the header's iteration bounds.  CPU only.  python scratch/dist_iterations.py"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
out = os.path.join(HERE, "tmp")
os.makedirs(out, exist_ok=True)
exe = os.path.join(out, "dist_iterations")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-fast-math", "-ffp-contract=off", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                       os.path.join(HERE, "dist_iterations.cpp"), "-o", exe])
subprocess.check_call([exe])
