"""Mirror of the reference's `data` package: only feature_loader is on this package's path."""
