from .csvm import CascadeSVM

__all__ = ["CascadeSVM"]
