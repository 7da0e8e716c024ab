"""What stream placement is worth: four k = 17 pipelines (tools/inflight_k17.py's measurement, "4") in three fresh processes -
  untouched   the pool as the engine primes it;
  foreign     N streams made by the host (hipStreamCreate) before the engine's first call;
  calibrated  the same, then zk_stream_placement mode 1.
Each row prints the placement report and inflight_k17's proofs/s line.  usage: placement_ab.py [N = 3] [repeats = 1]"""
import ctypes
import json
import os
import runpy
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def child(row, n):
    from webauthn_halo2_amd import engine as E

    E.load_library()
    if row != "untouched":
        with open("/proc/self/maps") as f:  # the HIP runtime the engine is linked against, as mapped
            hip = ctypes.CDLL({line.split()[-1] for line in f if "libamdhip64" in line}.pop())
        hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        for _ in range(n):
            s = ctypes.c_void_p()
            assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    report = E.stream_placement(0, calibrate=row == "calibrated")
    print(f"{row}: " + json.dumps({k: report[k] for k in ("n_queues", "flags", "ok", "calibrated", "main_queue", "streams", "probe_ms")}), flush=True)
    sys.argv = ["inflight_k17.py", "4"]
    runpy.run_path(os.path.join(HERE, "inflight_k17.py"), run_name="__main__")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
        sys.exit(0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    for _ in range(int(sys.argv[2]) if len(sys.argv) > 2 else 1):
        for row in ("untouched", "foreign", "calibrated"):
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", row, str(n)], timeout=600).returncode
            if rc:  # (nothing more is started on a device a child failed on)
                sys.exit(f"{row}: child exited {rc}")
