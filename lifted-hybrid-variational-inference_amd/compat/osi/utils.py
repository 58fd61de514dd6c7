"""Drop-in alias of the reference's ``osi/utils.py``: re-exports lhvi.utils."""
from lhvi.utils import *  # noqa: F401,F403
