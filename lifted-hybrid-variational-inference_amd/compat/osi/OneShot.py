"""Drop-in alias of the reference's ``osi/OneShot.py``: re-exports lhvi.oneshot.  ``LiftedOneShot2``,
``init_grid``, ``grad_check`` and TensorFlow's random start are not provided (docs/widened_rows.md)."""
from lhvi.oneshot import OneShot, LiftedOneShot  # noqa: F401
