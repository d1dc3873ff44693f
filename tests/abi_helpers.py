"""include/vlsa_hip.h as the ABI tests read it: the text without comments, and the declared names found by a regex of their own.
Deliberately NOT the header reader of vlsa_amd/_native.py: "declared and bound" would otherwise compare that reader with itself."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_PATH = os.path.join(ROOT, "include", "vlsa_hip.h")
with open(HEADER_PATH) as _f:
    HEADER_TEXT = re.sub(r"/\*.*?\*/", "", _f.read(), flags=re.S)


def declared_symbols():
    return sorted(set(re.findall(r"\b(vlsa_[a-z0-9_]+)\s*\(", HEADER_TEXT)))
