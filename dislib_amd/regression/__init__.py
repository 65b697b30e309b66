from dislib_amd.regression.forest import RandomForestRegressor
from dislib_amd.regression.linear import LinearRegression

__all__ = ['LinearRegression', 'RandomForestRegressor']
