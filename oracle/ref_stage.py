"""Recipe of what build() places under oracle/_ref/ (never committed): the reference's own Python modules that
tests/test_dropin_reference.py executes with this repository's engine behind dynamo's name.  The reference is pure Python,
so nothing is compiled; the files are copied from the reference checkout (``MVF_REFERENCE_TREE``, default below) when it
is readable, so that the test reads nothing outside the repository.  Where it is not, nothing is staged and the test skips."""
import os
import shutil

REFERENCE_TREE = os.environ.get("MVF_REFERENCE_TREE", "/root/reference")
STAGE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ref")
FILES = (
    "spateo/tdr/interpolations/utils.py",
    "spateo/tdr/interpolations/interpolation_sparseVFC.py",
    "spateo/tdr/morphometrics/morphofield/sparsevfc.py",
    "spateo/tdr/morphometrics/morphofield/gaussian_process.py",
    "spateo/tdr/morphometrics/morphofield_dg/GPVectorField.py",
    "spateo/tdr/morphometrics/morphofield_dg/differential_geometry.py",
)


def staged():
    return all(os.path.isfile(os.path.join(STAGE, f)) for f in FILES)


def stage():
    """Copy FILES from the reference checkout into oracle/_ref/ (same relative paths); True if all are there afterwards."""
    for f in FILES:
        src = os.path.join(REFERENCE_TREE, f)
        if not os.access(src, os.R_OK):
            return staged()
        dst = os.path.join(STAGE, f)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        shutil.copyfile(src, dst)
    return staged()
