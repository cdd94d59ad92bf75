"""One function of the test suite in a fresh child process on the ordered-reduction build (libdwiseneuro_hip_det.so,
DWN_DETERMINISTIC=1): what the tests/test_gpu_*_det.py modules compare this process against."""
import json
import os
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def deterministic_child(target):
    """Runs tests/det_call_worker.py on `target` ("module:function", a function without arguments whose result is JSON) with
    DWN_DETERMINISTIC=1 and without DWN_LIB_PATH.  Returns (the child's DWN_DETERMINISTIC, the file name of the library it loaded,
    the function's result: a tuple comes back as a list); the caller asserts on all three."""
    env = dict(os.environ, DWN_DETERMINISTIC="1")
    env.pop("DWN_LIB_PATH", None)
    res = subprocess.run([sys.executable, str(ROOT / "tests" / "det_call_worker.py"), target], cwd=str(ROOT), env=env,
                         capture_output=True, text=True, timeout=300)
    m = re.search(r"DET_CALL (\S+) deterministic=(\d) lib=(\S+) result=(.*)", res.stdout)
    assert res.returncode == 0 and m and m.group(1) == target, res.stdout[-2000:] + res.stderr[-3000:]
    print(m.group(0))
    return m.group(2), m.group(3), json.loads(m.group(4))
