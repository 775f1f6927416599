import os
import sys

import pytest

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO_ROOT not in sys.path:
    sys.path.insert(0, REPO_ROOT)

def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: requires an MI355X GPU")
    config.addinivalue_line(
        "markers",
        "reference: parity with the reference planner, checked against the "
        "results recorded under tests/golden/reference (run live against a "
        "reference checkout when METIS_REFERENCE_DIR names one)",
    )


@pytest.fixture(scope="session")
def data_dir():
    return os.path.join(REPO_ROOT, "tests", "data")


@pytest.fixture(scope="session")
def sample_profile_dir():
    """Synthetic MI355X-shaped sample profiles generated for tests."""
    return os.path.join(REPO_ROOT, "tests", "data", "profiles_synth")
