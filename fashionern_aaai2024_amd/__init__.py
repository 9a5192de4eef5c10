def __getattr__(name):      # the host layer's public classes, imported on first use (importing the package loads neither torch nor the library)
    if name in ("LiveGallery", "SlotTable"):
        from . import live_gallery
        return getattr(live_gallery, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
