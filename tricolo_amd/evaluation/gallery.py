"""A shape gallery: embed shapes once, keep the matrix where it is, ask for the top k of some text embeddings.

compute_metrics (eval_retrieval.py) rebuilds its matrices from per-caption tuples on every call; a ShapeGallery holds the
[Ns, D] float32 shape embeddings on the device they were given on, with the model id (and category) of every row, and ranks
queries against them:

    gallery, labels = ShapeGallery.from_captions(model_ids, categories, net.encode_shapes(batch))
    idx, sim, ids = gallery.query(net.encode_text(batch), k=5)
    idx, sim, ids, first_hit = gallery.rank(net.encode_text(batch), labels, k=5)

The order is the reference's (eval_retrieval.py:70-82): float64 dot products, larger first, equal similarities with the HIGHER shape
index first; first_hit[q] is the number of shapes ranking before shape labels[q] (MRR = mean 1 / (first_hit + 1)).  GPU tensors go
through ops.retrieval_gallery (csrc/gallery.hip): any number of shapes, k <= 64, D <= 4096.  On CPU tensors the same functions run a
float64 torch restatement of that order (a stable ascending argsort, flipped); it exists so that the interface and the ranking rule
can be used and tested without a GPU, is not tuned (it holds the whole [Nq, Ns] similarity matrix), and its similarities are torch's
matmul sums, not bit-equal to the kernel's.

CaptionGallery (below) is the other direction: the captions are kept, shapes ask, and several captions are correct for a shape.
"""
import numpy as np
import torch


class ShapeGallery:
    def __init__(self, embeddings, model_ids, categories=None):
        if embeddings.dim() != 2 or embeddings.dtype != torch.float32:
            raise ValueError("ShapeGallery: embeddings must be a float32 [Ns, D] tensor")
        model_ids = [str(m) for m in model_ids]
        if len(model_ids) != embeddings.shape[0]:
            raise ValueError(f"ShapeGallery: {embeddings.shape[0]} embeddings for {len(model_ids)} model ids")
        if categories is not None and len(categories) != len(model_ids):
            raise ValueError(f"ShapeGallery: {len(categories)} categories for {len(model_ids)} model ids")
        self.embeddings = embeddings.detach().contiguous()
        self.model_ids = model_ids
        self.categories = None if categories is None else [str(c) for c in categories]

    def __len__(self):
        return len(self.model_ids)

    @property
    def device(self):
        return self.embeddings.device

    @classmethod
    def from_captions(cls, model_ids, categories, shape_features, dataset=None):
        """Per-caption rows -> (gallery, labels int64 [rows]) by the rule of construct_embeddings_matrix: the FIRST row of each model id
        supplies its embedding, labels[i] is the gallery row of caption i; for dataset == "Primitives" the category is the key (and
        the model id takes the category's place).  The strings are de-duplicated on the host, the rows gathered where they are."""
        if shape_features.shape[0] != len(model_ids) or len(categories) != len(model_ids):
            raise ValueError("from_captions: model_ids, categories and shape_features must have one entry per caption")
        keys, others = (categories, model_ids) if dataset == "Primitives" else (model_ids, categories)
        label_of, first_rows = {}, []
        labels = np.zeros(len(keys), dtype=np.int64)
        for i, key in enumerate(keys):
            if key not in label_of:
                label_of[key] = len(first_rows)
                first_rows.append(i)
            labels[i] = label_of[key]
        rows = torch.tensor(first_rows, dtype=torch.int64, device=shape_features.device)
        emb = shape_features.detach().to(torch.float32).index_select(0, rows)
        return cls(emb, [keys[i] for i in first_rows], [others[i] for i in first_rows]), labels

    # ------------------------------------------------------------------------------------------------ ranking
    def _rank(self, text_features, labels, k):
        text = text_features.detach().to(torch.float32).contiguous()
        if text.dim() != 2 or text.shape[1] != self.embeddings.shape[1]:
            raise ValueError(f"ShapeGallery: queries must be [Nq, {self.embeddings.shape[1]}]")
        if text.device != self.device:
            raise ValueError(f"ShapeGallery: queries on {text.device}, gallery on {self.device}")
        if not 1 <= k <= len(self):
            raise ValueError("ShapeGallery: need 1 <= k <= number of shapes")
        lab = None
        if labels is not None:
            lab = torch.as_tensor(np.asarray(labels.cpu() if torch.is_tensor(labels) else labels), dtype=torch.int64)
            if lab.shape != (text.shape[0],) or (lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= len(self))):
                raise ValueError("ShapeGallery: one label in [0, number of shapes) per query")
        if text.is_cuda:
            from .. import ops
            idx, sim, hit = ops.retrieval_gallery(text, self.embeddings, None if lab is None else lab.to(torch.int32).to(self.device), k)
            return idx.long(), sim, None if hit is None else hit.long()
        sims = text.double() @ self.embeddings.double().t()
        order = torch.flip(torch.argsort(sims, dim=1, stable=True), dims=(1,))
        top = order[:, :k].contiguous()
        hit = None if lab is None else (order == lab[:, None]).to(torch.int64).argmax(dim=1)
        return top, torch.gather(sims, 1, top), hit

    def _ids(self, idx):
        return [[self.model_ids[j] for j in row] for row in idx.cpu().tolist()]

    def query(self, text_features, k=5):
        """-> (indices [Nq,k] int64, similarities [Nq,k] float64, model ids [Nq][k]) of the k best shapes per query, best first."""
        idx, sim, _ = self._rank(text_features, None, k)
        return idx, sim, self._ids(idx)

    def rank(self, text_features, labels, k=5):
        """query() plus first_hit [Nq] int64: how many shapes rank before shape labels[q]."""
        idx, sim, hit = self._rank(text_features, labels, k)
        return idx, sim, self._ids(idx), hit

    # ------------------------------------------------------------------------------------------------ storage
    def save(self, path):
        """An .npz of embeddings (float32), model_ids and categories (strings; an empty array when there are none)."""
        with open(path, "wb") as f:
            np.savez(f, embeddings=self.embeddings.cpu().numpy(), model_ids=np.array(self.model_ids, dtype=str),
                     categories=np.array(self.categories if self.categories is not None else [], dtype=str))

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as z:
            emb = torch.from_numpy(z["embeddings"])
            ids, cats = z["model_ids"].tolist(), z["categories"].tolist()
        if device is not None:
            emb = emb.to(device)
        return cls(emb, ids, cats if len(cats) == len(ids) and len(ids) > 0 else None)


class CaptionGallery:
    """The other direction: caption embeddings kept where they are, shapes ask.  Several captions are correct for a shape, so a caption
    carries a CLASS - the gallery row of its shape, the label ShapeGallery.from_captions gives it (negative: no shape) - and a query
    names one:

        captions = CaptionGallery.from_captions(model_ids, categories, net.encode_text(batch))
        idx, sim = captions.query(shapes.embeddings, k=5)
        idx, sim, first_hit = captions.rank(shapes.embeddings, torch.arange(len(shapes)), k=5)

    The order is ShapeGallery's (float64 dot products, larger first, equal similarities with the HIGHER caption index first).
    first_hit[q] is the position of the first caption of class shape_labels[q] in that order - the number of captions ranking before
    the best correct one, MRR = mean 1 / (first_hit + 1) - and -1 when no caption has that class.  GPU tensors go through
    ops.retrieval_classes (csrc/gallery.hip: the kernel of ops.retrieval_gallery, the same bits); CPU tensors through the float64 torch
    restatement, which is as untuned as ShapeGallery's and exists for the interface and the tests."""

    def __init__(self, embeddings, classes, model_ids=None, categories=None, captions=None):
        if embeddings.dim() != 2 or embeddings.dtype != torch.float32:
            raise ValueError("CaptionGallery: embeddings must be a float32 [Nt, D] tensor")
        n = embeddings.shape[0]
        classes = torch.as_tensor(np.asarray(classes.cpu() if torch.is_tensor(classes) else classes), dtype=torch.int64)
        if classes.shape != (n,):
            raise ValueError(f"CaptionGallery: {n} embeddings need {n} classes")
        for name, column in (("model ids", model_ids), ("categories", categories), ("captions", captions)):
            if column is not None and len(column) != n:
                raise ValueError(f"CaptionGallery: {n} embeddings for {len(column)} {name}")
        self.embeddings = embeddings.detach().contiguous()
        self.classes = classes                                         # on the host; the device copy lives in the CSR
        self.model_ids = None if model_ids is None else [str(m) for m in model_ids]
        self.categories = None if categories is None else [str(c) for c in categories]
        self.captions = None if captions is None else [str(c) for c in captions]
        self.num_classes = max(int(classes.max()) + 1, 0) if n else 0
        self._csr = None

    def __len__(self):
        return self.embeddings.shape[0]

    @property
    def device(self):
        return self.embeddings.device

    @classmethod
    def from_captions(cls, model_ids, categories, text_features, dataset=None, captions=None):
        """Per-caption rows -> gallery: every row stays a candidate, its class is the label ShapeGallery.from_captions gives it (the
        order of first occurrence of its model id; of its category for dataset == "Primitives")."""
        if text_features.shape[0] != len(model_ids) or len(categories) != len(model_ids):
            raise ValueError("from_captions: model_ids, categories and text_features must have one entry per caption")
        keys = categories if dataset == "Primitives" else model_ids
        label_of = {}
        classes = np.array([label_of.setdefault(key, len(label_of)) for key in keys], dtype=np.int64)
        return cls(text_features.detach().to(torch.float32), classes, model_ids, categories, captions)

    # ------------------------------------------------------------------------------------------------ ranking
    def _rank(self, shape_features, labels, k):
        query = shape_features.detach().to(torch.float32).contiguous()
        if query.dim() != 2 or query.shape[1] != self.embeddings.shape[1]:
            raise ValueError(f"CaptionGallery: queries must be [Nq, {self.embeddings.shape[1]}]")
        if query.device != self.device:
            raise ValueError(f"CaptionGallery: queries on {query.device}, gallery on {self.device}")
        if not 1 <= k <= len(self):
            raise ValueError("CaptionGallery: need 1 <= k <= number of captions")
        lab = None
        if labels is not None:
            lab = torch.as_tensor(np.asarray(labels.cpu() if torch.is_tensor(labels) else labels), dtype=torch.int64)
            if lab.shape != (query.shape[0],):
                raise ValueError("CaptionGallery: one shape label per query")
        if query.is_cuda:
            from .. import ops
            if lab is None:
                idx, sim, _ = ops.retrieval_classes(query, self.embeddings, k=k)
                return idx.long(), sim, None
            if self._csr is None:
                self._csr = ops.class_csr(self.classes.to(self.device), self.num_classes)
            off, rows, ncls = self._csr
            # a label past int32 names no class either way
            q32 = lab.clamp(-1, 2**31 - 1).to(torch.int32).to(self.device)
            idx, sim, hit = ops.retrieval_classes_csr(query, self.embeddings, q32, off, rows, ncls, k)
            return idx.long(), sim, hit.long()
        sims = query.double() @ self.embeddings.double().t()
        order = torch.flip(torch.argsort(sims, dim=1, stable=True), dims=(1,))
        top = order[:, :k].contiguous()
        hit = None
        if lab is not None:
            rel = (self.classes[order] == lab[:, None]) & (lab[:, None] >= 0)
            hit = torch.where(rel.any(dim=1), rel.to(torch.int64).argmax(dim=1), torch.full_like(lab, -1))
        return top, torch.gather(sims, 1, top), hit

    def query(self, shape_features, k=5):
        """-> (indices [Nq,k] int64, similarities [Nq,k] float64) of the k best captions per shape, best first."""
        idx, sim, _ = self._rank(shape_features, None, k)
        return idx, sim

    def rank(self, shape_features, shape_labels, k=5):
        """query() plus first_hit [Nq] int64: how many captions rank before the best caption of shape shape_labels[q]; -1: it has none."""
        return self._rank(shape_features, shape_labels, k)

    # ------------------------------------------------------------------------------------------------ storage
    def save(self, path):
        """ShapeGallery's .npz (embeddings, model_ids, categories: one row per caption here) plus classes (int64) and captions; a column
        that is not held is an empty array."""
        def column(c):
            return np.array(c if c is not None else [], dtype=str)
        with open(path, "wb") as f:
            np.savez(f, embeddings=self.embeddings.cpu().numpy(), model_ids=column(self.model_ids), categories=column(self.categories),
                     classes=self.classes.numpy(), captions=column(self.captions))

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as z:
            emb, classes = torch.from_numpy(z["embeddings"]), z["classes"]
            ids, cats, caps = (z[name].tolist() for name in ("model_ids", "categories", "captions"))
        if device is not None:
            emb = emb.to(device)
        n = emb.shape[0]
        return cls(emb, classes, *(c if len(c) == n and n > 0 else None for c in (ids, cats, caps)))
