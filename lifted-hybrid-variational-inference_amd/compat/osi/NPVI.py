"""Drop-in alias of the reference's ``osi/NPVI.py``: re-exports lhvi.npvi.  ``isotropic_cov``, ``LiftedNPVI2``,
``init_grid`` and TensorFlow's random start are not provided (docs/widened_rows.md)."""
from lhvi.npvi import NPVI, LiftedNPVI  # noqa: F401
