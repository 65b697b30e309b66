from dislib_amd.preprocessing.classes import StandardScaler

__all__ = ['StandardScaler']
