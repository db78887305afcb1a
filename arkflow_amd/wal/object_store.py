"""Object-store drivers under the segmented WAL (wal/segment_store.py).

Two drivers share one small interface — ``put`` (optionally conditional),
``get``, ``list``, ``delete``:

- ``DirObjectStore``: a local directory, one file per object. The ETag is
  the MD5 of the content (as S3 reports for single-part objects), so there
  is no side-car metadata to go stale. Writes are tmp-file + rename;
  conditional PUTs are serialized with a per-directory thread lock plus an
  flock on the directory for writers in other processes.
- ``S3ObjectStore``: any S3-compatible endpoint (path-style addressing, so
  MinIO works) through a stdlib-only SigV4 client — no boto3.

Conditional PUTs follow HTTP semantics: ``if_none_match=True`` sends
``If-None-Match: *`` (create only), ``if_match=<etag>`` sends ``If-Match``
(replace only that version). A failed precondition raises
``PreconditionFailed``; the manifest writer reloads, merges and retries.
"""
from __future__ import annotations

import datetime
import fcntl
import hashlib
import hmac
import os
import threading
import urllib.error
import urllib.parse
import urllib.request
import uuid
import xml.etree.ElementTree as ET
from typing import Dict, List, Optional, Tuple


class PreconditionFailed(Exception):
    """A conditional PUT lost: the object exists (If-None-Match: *) or its
    ETag moved on (If-Match)."""


def _etag(data: bytes) -> str:
    return hashlib.md5(data).hexdigest()


# ---------------------------------------------------------------- directory
_dir_locks: Dict[str, threading.Lock] = {}
_dir_locks_guard = threading.Lock()


def _dir_lock(root: str) -> threading.Lock:
    with _dir_locks_guard:
        return _dir_locks.setdefault(root, threading.Lock())


class DirObjectStore:
    """Directory-backed object store (the CI / single-node driver)."""

    def __init__(self, root: str):
        self.root = os.path.abspath(root)
        os.makedirs(self.root, exist_ok=True)
        self._lock = _dir_lock(self.root)

    def _path(self, key: str) -> str:
        path = os.path.normpath(os.path.join(self.root, key))
        if not path.startswith(self.root + os.sep):
            raise ValueError(f"object key escapes the store: {key!r}")
        return path

    def _read(self, path: str) -> Optional[bytes]:
        try:
            with open(path, "rb") as f:
                return f.read()
        except (FileNotFoundError, IsADirectoryError):
            return None

    def put(self, key: str, data: bytes, if_match: Optional[str] = None,
            if_none_match: bool = False) -> str:
        path = self._path(key)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        tmp = os.path.join(os.path.dirname(path),
                           f".tmp-{uuid.uuid4().hex}")
        with self._lock:
            dfd = os.open(self.root, os.O_RDONLY)
            try:
                fcntl.flock(dfd, fcntl.LOCK_EX)
                if if_none_match or if_match is not None:
                    cur = self._read(path)
                    if if_none_match and cur is not None:
                        raise PreconditionFailed(key)
                    if if_match is not None and (
                            cur is None or _etag(cur) != if_match):
                        raise PreconditionFailed(key)
                with open(tmp, "wb") as f:
                    f.write(data)
                    f.flush()
                    os.fsync(f.fileno())
                os.replace(tmp, path)
            finally:
                os.close(dfd)  # drops the flock
        return _etag(data)

    def get(self, key: str) -> Optional[Tuple[bytes, str]]:
        data = self._read(self._path(key))
        if data is None:
            return None
        return data, _etag(data)

    def list(self, prefix: str = "") -> List[str]:
        out = []
        for dirpath, _, files in os.walk(self.root):
            for name in files:
                if name.startswith(".tmp-"):
                    continue
                rel = os.path.relpath(os.path.join(dirpath, name), self.root)
                rel = rel.replace(os.sep, "/")
                if rel.startswith(prefix):
                    out.append(rel)
        return sorted(out)

    def delete(self, key: str) -> None:
        try:
            os.remove(self._path(key))
        except FileNotFoundError:
            pass


# ----------------------------------------------------------------------- s3
def _quote(s: str, safe: str = "") -> str:
    return urllib.parse.quote(s, safe="-_.~" + safe)


class S3ObjectStore:
    """S3-compatible driver: SigV4-signed path-style requests over urllib."""

    def __init__(self, endpoint: str, bucket: str, prefix: str = "",
                 access_key: Optional[str] = None,
                 secret_key: Optional[str] = None,
                 region: str = "us-east-1", timeout: float = 60.0):
        if not endpoint:
            raise ValueError("S3ObjectStore needs an endpoint "
                             "(config or MINIO_ENDPOINT / S3_ENDPOINT)")
        if "://" not in endpoint:
            endpoint = "http://" + endpoint
        self.endpoint = endpoint.rstrip("/")
        self.bucket = bucket
        self.prefix = prefix.strip("/")
        self.access_key = access_key \
            or os.environ.get("AWS_ACCESS_KEY_ID") \
            or os.environ.get("MINIO_ACCESS_KEY", "minioadmin")
        self.secret_key = secret_key \
            or os.environ.get("AWS_SECRET_ACCESS_KEY") \
            or os.environ.get("MINIO_SECRET_KEY", "minioadmin")
        self.region = region
        self.timeout = timeout
        self._host = urllib.parse.urlsplit(self.endpoint).netloc

    @classmethod
    def from_env(cls, bucket: str, prefix: str = "") -> "S3ObjectStore":
        return cls(os.environ.get("MINIO_ENDPOINT")
                   or os.environ.get("S3_ENDPOINT", ""), bucket, prefix,
                   region=os.environ.get("AWS_REGION", "us-east-1"))

    # ------------------------------------------------------------- signing
    def _full_key(self, key: str) -> str:
        return f"{self.prefix}/{key}" if self.prefix else key

    def _sign(self, method: str, path: str, query: Dict[str, str],
              body: bytes) -> Tuple[str, Dict[str, str]]:
        now = datetime.datetime.now(datetime.timezone.utc)
        amz_date = now.strftime("%Y%m%dT%H%M%SZ")
        day = now.strftime("%Y%m%d")
        payload_hash = hashlib.sha256(body).hexdigest()
        canon_uri = _quote(path, safe="/")
        canon_query = "&".join(
            f"{_quote(k)}={_quote(v)}" for k, v in sorted(query.items()))
        headers = {"host": self._host,
                   "x-amz-content-sha256": payload_hash,
                   "x-amz-date": amz_date}
        signed = ";".join(sorted(headers))
        canon_headers = "".join(f"{k}:{headers[k]}\n"
                                for k in sorted(headers))
        canon_req = "\n".join([method, canon_uri, canon_query,
                               canon_headers, signed, payload_hash])
        scope = f"{day}/{self.region}/s3/aws4_request"
        to_sign = "\n".join(["AWS4-HMAC-SHA256", amz_date, scope,
                             hashlib.sha256(canon_req.encode()).hexdigest()])

        def h(key: bytes, msg: str) -> bytes:
            return hmac.new(key, msg.encode(), hashlib.sha256).digest()

        k = h(("AWS4" + self.secret_key).encode(), day)
        for part in (self.region, "s3", "aws4_request"):
            k = h(k, part)
        sig = hmac.new(k, to_sign.encode(), hashlib.sha256).hexdigest()
        headers["authorization"] = (
            f"AWS4-HMAC-SHA256 Credential={self.access_key}/{scope}, "
            f"SignedHeaders={signed}, Signature={sig}")
        url = self.endpoint + canon_uri
        if canon_query:
            url += "?" + canon_query
        return url, headers

    def _request(self, method: str, path: str,
                 query: Optional[Dict[str, str]] = None, body: bytes = b"",
                 extra: Optional[Dict[str, str]] = None,
                 ok_status: Tuple[int, ...] = ()):
        """→ (status, headers, body). HTTP errors outside ``ok_status``
        raise OSError."""
        url, headers = self._sign(method, path, query or {}, body)
        headers.update(extra or {})
        req = urllib.request.Request(
            url, data=body if method in ("PUT", "POST") else None,
            headers=headers, method=method)
        try:
            with urllib.request.urlopen(req, timeout=self.timeout) as r:
                return r.status, r.headers, r.read()
        except urllib.error.HTTPError as e:
            data = e.read()
            if e.code in ok_status:
                return e.code, e.headers, data
            raise OSError(f"s3 {method} {path}: HTTP {e.code} "
                          f"{data[:200]!r}") from e

    # ----------------------------------------------------------- interface
    def ensure_bucket(self) -> None:
        # 409 = BucketAlreadyOwnedByYou / BucketAlreadyExists
        self._request("PUT", f"/{self.bucket}", ok_status=(409,))

    def put(self, key: str, data: bytes, if_match: Optional[str] = None,
            if_none_match: bool = False) -> str:
        extra = {}
        if if_none_match:
            extra["If-None-Match"] = "*"
        if if_match is not None:
            extra["If-Match"] = if_match
        status, headers, _ = self._request(
            "PUT", f"/{self.bucket}/{self._full_key(key)}", body=data,
            extra=extra, ok_status=(409, 412))
        if status in (409, 412):  # 409: ConditionalRequestConflict
            raise PreconditionFailed(key)
        return (headers.get("ETag") or _etag(data)).strip('"')

    def get(self, key: str) -> Optional[Tuple[bytes, str]]:
        status, headers, data = self._request(
            "GET", f"/{self.bucket}/{self._full_key(key)}",
            ok_status=(404,))
        if status == 404:
            return None
        return data, (headers.get("ETag") or _etag(data)).strip('"')

    def list(self, prefix: str = "") -> List[str]:
        full = self._full_key(prefix)
        strip = len(self.prefix) + 1 if self.prefix else 0
        out: List[str] = []
        token = None
        while True:
            query = {"list-type": "2", "prefix": full}
            if token:
                query["continuation-token"] = token
            _, _, data = self._request("GET", f"/{self.bucket}", query)
            root = ET.fromstring(data)
            truncated, token = False, None
            for el in root.iter():
                tag = el.tag.rsplit("}", 1)[-1]  # drop the xml namespace
                if tag == "Key" and el.text:
                    out.append(el.text[strip:])
                elif tag == "IsTruncated":
                    truncated = (el.text or "").strip() == "true"
                elif tag == "NextContinuationToken":
                    token = el.text
            if not truncated or not token:
                break
        return sorted(out)

    def delete(self, key: str) -> None:
        self._request("DELETE", f"/{self.bucket}/{self._full_key(key)}",
                      ok_status=(404,))
