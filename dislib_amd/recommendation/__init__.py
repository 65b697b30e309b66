from dislib_amd.recommendation.als import ALS

__all__ = ['ALS']
