"""Drop-in alias package for the reference `data` package."""
