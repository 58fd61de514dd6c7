"""Drop-in alias of the reference's ``osi`` package: ``import osi.utils as utils`` resolves here."""
