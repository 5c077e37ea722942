"""The ABI number, pinned once: the header's define, the bindings' constant and what the built library reports."""
import os
import re

from foley_amd.host import runtime as rt

ABI_VERSION = 13
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "foley_hip.h")


def assert_abi_version():
    assert re.search(r"#define FOLEY_ABI_VERSION %d\b" % ABI_VERSION, open(HEADER).read())
    assert rt.load_library().foley_abi_version() == rt.ABI_VERSION == ABI_VERSION
