"""The case functions of tests/test_exports_edges.py on the GPU: every caller-side export of the C ABI at the same strided and
ragged shapes, both precisions, the same NumPy longdouble references and derived bounds; and the row limit -- 65539 rows are more
than one launch may put on gridDim.y, which only the hardware enforces."""
import pytest

from test_exports_edges import CASES, _rejection_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("export", list(CASES))
def test_export_at_its_edges_on_the_gpu(hip_library, export, precision):
    CASES[export](hip_library, precision)


@pytest.mark.parametrize("precision", [64, 32])
def test_bad_shapes_are_refused_before_any_launch_on_the_gpu(hip_library, precision):
    _rejection_case(hip_library, precision)
