"""The library sources hold the product only: timing probes and ablation kernels live as patch files under tools/probes/ (DESIGN.md
section 3, "Probes"), not as #ifdef blocks or -D flags that one stray definition could ship."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gif_amd", "csrc")
CONDITIONAL = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$")
DEVICE_ONLY = re.compile(r"^\s*defined\s*\(\s*__HIP_DEVICE_COMPILE__\s*\)\s*(//.*)?$")


def test_only_device_compile_conditionals_and_no_gif_defines():
    sources = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert {"common.h", "conv_igemm.hip", "conv_wgrad.hip", "conv_winograd.hip"} <= {os.path.basename(p) for p in sources}, sources
    bad = []
    for path in sources:
        with open(path) as f:
            for no, text in enumerate(f, 1):
                m = CONDITIONAL.match(text)
                if m and not (m.group(1) == "if" and DEVICE_ONLY.match(m.group(2))):
                    bad.append(f"{os.path.basename(path)}:{no}: {text.strip()}")
    assert not bad, "preprocessor conditionals other than '#if defined(__HIP_DEVICE_COMPILE__)':\n" + "\n".join(bad)
    with open(os.path.join(CSRC, "Makefile")) as f:
        make = f.read()
    assert re.search(r"^CXXFLAGS\s*[:+?]?=", make, re.M), "the Makefile no longer sets CXXFLAGS: update this test"
    assert "-DGIF_" not in make, "the Makefile passes a -DGIF_ flag"
