from dislib_amd.cluster.dbscan import DBSCAN
from dislib_amd.cluster.gm import GaussianMixture
from dislib_amd.cluster.kmeans import KMeans

__all__ = ['KMeans', 'GaussianMixture', 'DBSCAN']
