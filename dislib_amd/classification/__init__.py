from .csvm import CascadeSVM
from .logreg import LogisticRegression
from .rf import RandomForestClassifier

__all__ = ["CascadeSVM", "LogisticRegression", "RandomForestClassifier"]
