"""Kernel names of the built library's gfx950 code objects (symbol names only), shared by the CPU tests that read them."""
import os
import re
import shutil
import subprocess

import pytest

from llama2_ts_amd import runtime


def kernel_names(tmp):
    """Build, unbundle the library's device code into `tmp` and return the mangled names of every gfx950 kernel."""
    import __graft_entry__ as graft
    graft.build()
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("no ROCm llvm tools here")
    so = tmp / "lib.so"
    shutil.copy(runtime.LIB_PATH, so)
    subprocess.run([objdump, "--offloading", str(so)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=str(tmp))
    names = set()
    for o in os.listdir(tmp):
        if "gfx950" in o:
            notes = subprocess.check_output([readelf, "--notes", str(tmp / o)]).decode()
            names |= set(re.findall(r"\.name:\s+(_Z\S+)", notes))
    return names
