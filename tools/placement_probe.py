"""The stream placement of a device as the engine measures it (zk_stream_placement), as one JSON line.
usage: placement_probe.py [device] [--calibrate]      exit status 1 when the report is not OK"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from webauthn_halo2_amd import engine as E  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
report = E.stream_placement(int(args[0]) if args else 0, calibrate="--calibrate" in sys.argv)
print(json.dumps(report))
sys.exit(0 if report["ok"] else 1)
