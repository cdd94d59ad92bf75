"""Child process of tests/det_child.py: imports the function named on the command line as module:function, calls it with whatever
library DWN_DETERMINISTIC selects and prints one line: the DWN_DETERMINISTIC value, the loaded library's file name and the
function's result as JSON."""
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402

import sensorium_amd._lib as L  # noqa: E402


def main():
    module, function = sys.argv[1].split(":")
    result = getattr(importlib.import_module(module), function)()
    print(f"DET_CALL {sys.argv[1]} deterministic={os.environ.get('DWN_DETERMINISTIC', '0')} lib={L.LIB_PATH.name} "
          f"result={json.dumps(result)}")


if __name__ == "__main__":
    main()
