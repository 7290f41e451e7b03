from .AutoEncoder import WholeBodyAE
from .Whole_body_hybrid import Wholebody

__all__ = ["WholeBodyAE", "Wholebody"]
