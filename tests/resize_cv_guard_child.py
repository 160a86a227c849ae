"""Child runner of tests/test_resize_cv.py: ``python -m tests.resize_cv_guard_child resize_cv``.  Importing that module registers its cases in the
table of tests/test_operand_containment.py; everything else is tests/operand_guard_child.py."""
from __future__ import annotations

import sys

from tests import test_resize_cv  # noqa: F401  (registers the ``resize_cv`` family)
from tests.operand_guard_child import main

if __name__ == "__main__":
    sys.exit(main())
