from dislib_amd.decomposition.pca import PCA

__all__ = ['PCA']
