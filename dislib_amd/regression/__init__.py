from dislib_amd.regression.linear import LinearRegression

__all__ = ['LinearRegression']
