from .detection_head import DetectionHead  # noqa: F401
