"""Worker of test_gpu_summarise_patterns.py: summarisePatterns over both fixtures in a fresh process, under the EPIHIP_*
hooks the parent put in the environment (the switches are read once per process).  Prints one line per call: the digest of
its Reports and the call's statistics."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import test_gpu_summarise_patterns as TS  # noqa: E402
import epialleler_amd as ea  # noqa: E402

for reps, st in TS.worker_reports(ea):
    print("summary", TS.digest(reps), st[0], st[1], st[2])
