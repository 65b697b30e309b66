from .csvm import CascadeSVM
from .rf import RandomForestClassifier

__all__ = ["CascadeSVM", "RandomForestClassifier"]
